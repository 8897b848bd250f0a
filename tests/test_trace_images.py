"""The walks that only run inside a render -- `walk_body`, `nee_body`'s inline
occlusion walk, the wavefront walk (rt0_integrator.h) -- on the hard meshes
of tests/test_trace.py, at image level: they are compiled per scene and
cannot be called from the ray-query hook.  Their node visit and choice of the
next node is the hook's own (`BvhWalk`, shared with `bvh_closest`); what is
theirs alone -- pending leaves, job and queue refills, the result stores --
shows only here.

Mask scenes: BASELINE config 5's scene with its model replaced by the cube, a
flat grid and the stadium, against the oracle's brute-force loop over every
triangle and between the render paths.  Hit-mask scenes: every pixel is one
closest-hit answer (three possible values), so a pixel may differ from the
oracle only next to a place where the oracle's own image changes value.
"""
import numpy as np
import pytest

import oracle as O
import rt0
from rt0 import meshes as M
from test_gpu_defer import close_and_mostly_identical
from test_models import cfg_by_name, pixel_match

SIZE = 48
# model-space meshes sized for an instance of scale 0.9 / 0.5 (the configs' own)
MASK_MESHES = {
    "cube": lambda: M.cube(0.6),
    "grid": lambda: M.quad_grid(32, axis=1, half=1.0, level=-0.25),
    "stadium": M.stadium,
}


def world(cfg, cfgs, models):
    """World triangles + owners of a config's TRIANGLE entries with the given models."""
    scene, sdf = rt0.scene_strings(cfg, cfgs)
    meshes, ne, ns, _ = rt0.parse_scene(scene, sdf)
    vs, owners = [], []
    for k, ((v, t), m) in enumerate(zip(models, meshes[ne + ns:])):
        w = M.world_triangles(v, t, list(m.pos), m.joker[0])
        vs.append(w)
        owners.append(np.full(len(w), k, np.int32))
    return np.concatenate(vs), np.concatenate(owners)


def oracle_with(cfg, cfgs, models, size=SIZE):
    o = O.Oracle(cfg, cfgs, width=size, height=size)
    o.set_triangles(*world(cfg, cfgs, models))
    return o


def renderer_with(cfg, cfgs, models, size=SIZE, jit=True):
    r = rt0.Renderer(size, size)
    r.set_jit(jit)
    rt0.configure(r, cfg, cfgs)
    for k, (v, t) in enumerate(models):
        r.set_model(k, v, t)
    return r


def restir_chain(r, n=3):
    S, Mn, A = [], [], []
    zero = np.zeros((r.height, r.width, 4), np.float32)
    for k in range(1, n + 1):
        r.write_accum(zero)
        r.render(k, 1)
        S.append(r.read_accum())
        m, a = r.read_restir(0)
        Mn.append(m)
        A.append(a)
    return np.stack(S), np.stack(Mn), np.stack(A)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", list(MASK_MESHES))
def test_c5_scene_with_hard_mesh(mesh, cfgs, gpu_required):
    """Config 5's scene (spectral, ReSTIR + MIS, 10 lights) around a hard
    mesh: the deferred pass kernel (walk_body answers the light-sampling
    occlusion rays), the inline one (nee_body's walk) and the wavefront rounds
    (wf_walk_body) agree at test_gpu_defer's bar, and each matches the
    oracle's brute-force chain at test_c5_matches_bruteforce_oracle's bar:
    >= 0.98 of the pixels within 1e-3, the mean within 5e-3, the reservoirs
    >= 0.97."""
    cfg = cfg_by_name(cfgs, "c5_spectral_models")
    models = [MASK_MESHES[mesh]()]
    So, Mo, Ao = oracle_with(cfg, cfgs, models).frames_restir(3)
    out = {}
    for label, defer, wf, path in (("deferred", True, 0, "deferred"), ("inline", False, 0, "pass"),
                                   ("wavefront", True, 2, "wavefront")):
        r = renderer_with(cfg, cfgs, models)
        r.set_defer_light_sampling(defer)
        r.set_wavefront(wf)
        out[label] = restir_chain(r)
        assert r.last_render_path() == path, (label, r.last_render_path())
        S, Mn, A = out[label]
        assert np.isfinite(S).all()
        for k in range(3):
            ok = pixel_match(S[k][..., :3], So[k][..., :3]).mean()
            okr = (pixel_match(Mn[k], Mo[k]) & pixel_match(A[k], Ao[k])).mean()
            dm = abs(S[k][..., :3].mean() - So[k][..., :3].mean())
            print("%s %s pass %d: pixels %.4f reservoirs %.4f mean diff %.2e" % (mesh, label, k + 1, ok, okr, dm))
            assert ok >= 0.98, (mesh, label, k, ok)
            assert dm <= 5e-3 * max(1.0, So[k][..., :3].mean()), (mesh, label, k, dm)
            assert okr >= 0.97, (mesh, label, k, okr)
    for other in ("inline", "wavefront"):
        s0, m0, a0 = out["deferred"]
        s1, m1, a1 = out[other]
        print("%s deferred vs %s: bit-identical samples %.4f reservoirs %.4f"
              % (mesh, other, (s0[..., :3] == s1[..., :3]).all(-1).mean(), (m0 == m1).all(-1).mean()))
        close_and_mostly_identical(m0, m1, "reservoir main")
        close_and_mostly_identical(a0, a1, "reservoir aux")
        close_and_mostly_identical(s0[..., :3], s1[..., :3], "samples")


@pytest.mark.gpu
def test_jit_matches_aot_on_cube_and_grid(cfgs, gpu_required):
    """tri_models with its two models replaced by the cube and the grid: the
    scene-specialised kernel (LDS treelet, 16-bit stack) and the
    ahead-of-time one find the same hits."""
    cfg = cfg_by_name(cfgs, "tri_models")
    models = [M.cube(0.6), M.quad_grid(32, axis=1, half=1.0, level=0.5)]
    a, b = (renderer_with(cfg, cfgs, models, jit=j) for j in (True, False))
    ref = oracle_with(cfg, cfgs, models).frame(2)[0]
    for r in (a, b):
        r.render(2, 1)
    ga, gb = a.read_accum(), b.read_accum()
    same = pixel_match(ga[..., :3], gb[..., :3]).mean()
    print("jit vs aot %.4f, vs oracle %.4f / %.4f" % (same, pixel_match(ga[..., :3], ref[..., :3]).mean(),
                                                      pixel_match(gb[..., :3], ref[..., :3]).mean()))
    assert same >= 0.98, same
    for g in (ga, gb):
        assert pixel_match(g[..., :3], ref[..., :3]).mean() >= 0.98


HIT_MASK_MESHES = ["cube", "grid_z", "stadium", "slivers", "concentric", "cube_degenerate", "triangle"]


def hit_mask_cfg(cfgs):
    """A black back plane, one model in MAT_LIGHT_4 and an icosphere(1) in
    MAT_LIGHT_CANDLE_4; one bounce, no light sampling: a pixel's sample is
    the emission of what its camera ray hits first."""
    base = cfg_by_name(cfgs, "tri_models")
    return dict(base, name="hit_mask", scene_lines=[
        "MAT_BLACK, PLANE, vec3(0.0, 0.0, 1.0), vec4(6.0, 0.0, 0.0, 0.0)",
        "MAT_LIGHT_4, TRIANGLE, vec3(0.0, 0.0, -0.5), vec4(0.8)",
        "MAT_LIGHT_CANDLE_4, TRIANGLE, vec3(0.6, 0.5, 0.8), vec4(0.25)"],
        constants={"MAX_BOUNCES": 1, "MAX_DIFF_BOUNCES": 1, "sample_lights": False}, defines={}, camera=None)


def near_change(img, reach=2):
    """Pixels within `reach` of a place where the image changes value."""
    ch = np.zeros(img.shape[:2], bool)
    dx = (img[:, 1:] != img[:, :-1]).any(-1)
    dy = (img[1:] != img[:-1]).any(-1)
    ch[:, 1:] |= dx
    ch[:, :-1] |= dx
    ch[1:] |= dy
    ch[:-1] |= dy
    out = ch.copy()
    for _ in range(reach):
        g = out.copy()
        g[1:] |= out[:-1]
        g[:-1] |= out[1:]
        g[:, 1:] |= out[:, :-1]
        g[:, :-1] |= out[:, 1:]
        g[1:, 1:] |= out[:-1, :-1]
        g[:-1, :-1] |= out[1:, 1:]
        g[1:, :-1] |= out[:-1, 1:]
        g[:-1, 1:] |= out[1:, :-1]
        out = g
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mesh", HIT_MASK_MESHES)
def test_hit_mask_matches_oracle_away_from_silhouettes(mesh, cfgs, gpu_required):
    """Passes 1-4 of a hit-mask scene: the oracle's image holds at most three
    values, and every pixel on which the GPU differs from it lies within two
    pixels of a change of value in the oracle's own image -- no pinhole in
    the interior of a model."""
    cfg = hit_mask_cfg(cfgs)
    models = [rt0.meshes.menagerie()[mesh], M.icosphere(1)]
    o = oracle_with(cfg, cfgs, models)
    r = renderer_with(cfg, cfgs, models)
    for k in range(1, 5):
        ref = o.frame(k)[0][..., :3]
        values = np.unique(ref.reshape(-1, 3), axis=0)
        assert len(values) <= 3, values
        r.clear()
        r.render(k, 1)
        got = r.read_accum()[..., :3]
        differ = ~pixel_match(got, ref)
        interior = differ & ~near_change(ref)
        print("%s pass %d: %d values, %d pixels differ, %d in the interior" % (mesh, k, len(values), differ.sum(),
                                                                              interior.sum()))
        assert not interior.any(), (mesh, k, np.argwhere(interior)[:5].tolist())

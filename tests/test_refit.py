"""Deforming triangle models: rt0_update_model* and the device-side BVH refit.

A refit keeps the tree's links and leaf order and recomputes every triangle
record and every box on the device from new vertex positions
(rt0_refit.hip).  Checked here:

1. the same positions again leave the device bytes as the build wrote them
   (`eps` is allowed 1 ulp; the refit rounds it as the tree's builder does --
   without FMA for the host builder, as k_pack for the device LBVH -- and the
   largest difference measured on the MI355X is 0 ulp on every mesh);
2. after a deformation the tree is the exact tree of the new geometry: every
   leaf-side box equals the float32 min/max of its triangle's world vertices,
   every inner-side box the union of that child's two boxes (equality, not
   containment), every TriDev the record of the new world vertices bit for
   bit, links / leaf order / depth / treelet untouched -- for both builders;
3. the walk on the refitted tree returns what the loop over every triangle
   returns (test_trace.py's criterion 1, no ray left out);
4. and what a context freshly built from the deformed model returns;
5. positions from a torch tensor on the GPU (no host round trip) give the
   same bytes, and survive a later rebuild;
6. the rendered image matches the brute-force oracle of the deformed model
   without a recompilation;
7. argument and state errors.

"Exact" is numpy float32: w = float32(pos) + float32(s) * p, rounded after the
multiply and after the add, as build_bvh's gather rounds.

Deformations: `smooth` (another amp / freq of the displaced icosphere; a fixed
shear plus a per-vertex sine offset elsewhere) and `hostile` (the vertex
positions permuted among themselves: boxes overlap everywhere, the tree is
terrible and must still be right).

CPU (no GPU): the height order the refit runs in (rt0_bvh_height_order).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import rt0
from rt0 import meshes as M

import test_models as TM
import test_trace as T

bits = T.bits
F32 = np.float32
N_RAYS = 4096


def quad():
    """Two triangles: one inner node."""
    v = np.array([(-1.0, -1.0, 0.1), (1.0, -1.0, -0.2), (1.0, 1.0, 0.3), (-1.0, 1.0, 0.0)], F32)
    return v, np.array([(0, 1, 2), (0, 2, 3)], np.int32)


MESHES = {
    "triangle": M.single_triangle(),
    "quad": quad(),
    "cube": M.cube(),
    "cube_degenerate": M.cube_with_degenerates(),
    "concentric": M.concentric(),
    "slivers": M.slivers(),
    "wavy3": M.wavy_icosphere(3),
}
NAMES = list(MESHES)
KINDS = ["smooth", "hostile"]
# one TRIANGLE instance at the origin with scale 1 (world = model space: the ray tests), and a placed, scaled one
UNIT = ((0.0, 0.0, 0.0), 1.0)
PLACED = ((0.3, -0.2, 0.1), 0.7)
TWO = [((0.45, -1.0, -1.7), 0.5), ((-0.5, -1.05, -1.3), 0.45)]  # the tri_models config's two instances


def scene_lines(insts):
    return [T.SCENE[0]] + ["MAT_CORNELL_WHITE, TRIANGLE, vec3(%r, %r, %r), vec4(%r, 0.0, 0.0, 0.0)" % (*p, s)
                           for p, s in insts]


def deformed(name, kind):
    v, _ = MESHES[name]
    v = np.asarray(v, F32)
    if kind == "identity":
        return v.copy()
    if kind == "hostile":
        return v[np.random.default_rng(11).permutation(len(v))].copy()
    if name == "wavy3":
        return M.wavy_icosphere(3, amp=0.13, freq=4.0)[0]
    a = np.array([[1.0, 0.2, 0.0], [0.0, 1.0, 0.15], [0.1, 0.0, 1.0]])
    p = v.astype(np.float64)
    off = 0.05 * np.sin(3.0 * p[:, [1, 2, 0]] + 0.37 * np.arange(len(p))[:, None])
    return (p @ a.T + off).astype(F32)


def world(v, inst):
    """float32 world vertices of an instance: two roundings per coordinate."""
    pos, s = inst
    return (np.asarray(pos, F32)[None, :] + (F32(s) * np.asarray(v, F32)).astype(F32)).astype(F32)


def context(models, insts, cull=()):
    """A 16x16 context with one TRIANGLE entry per model; `cull` = the
    entries with the back-face culling bit."""
    r = rt0.Renderer(16, 16)
    r.set_scene_glsl(rt0.scene_from_lines(scene_lines(insts))[0])
    if cull:
        meshes, ne, ns, lights = r.get_scene()
        for k in cull:
            meshes[ne + ns + k].mat_opts |= 8
        r.set_scene(meshes, ne, ns, len(meshes) - ne - ns, lights)
    for k, (v, t) in enumerate(models):
        r.set_model(k, v, t)
    return r


def topology(r):
    nodes, _, treelet = r.read_bvh()
    return (nodes["left"].copy(), nodes["right"].copy(), r.leaf_source(), r.model_info(), treelet)


def same_topology(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "a link changed"
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1]), "the leaf order changed"
    assert a[3] == b[3] and a[4] == b[4], "model_info or the treelet changed"


def leaf_world(r, models, insts):
    """[n, 3, 3] float32 world vertices of every leaf-order triangle, and its model."""
    lm, lt = r.leaf_source()
    w = np.zeros((len(lm), 3, 3), F32)
    for k, ((v, t), inst) in enumerate(zip(models, insts)):
        sel = lm == k
        w[sel] = world(v, inst)[np.asarray(t)[lt[sel]]]
    return w, lm


def assert_exact_tree(r, models, insts, cull=()):
    """Criterion 2 on the tree a context holds for `models`."""
    nodes, tris, _ = r.read_bvh()
    w, lm = leaf_world(r, models, insts)
    n = len(w)
    assert r.model_info()[0] == n == sum(len(t) for _, t in models)
    for k, (_, t) in enumerate(models):  # the leaves hold every triangle of every model once
        assert np.array_equal(np.sort(r.leaf_source()[1][lm == k]), np.arange(len(t)))
    e0, e1 = (w[:, 1] - w[:, 0]).astype(F32), (w[:, 2] - w[:, 0]).astype(F32)
    for got, want, what in ((tris["v0"], w[:, 0], "v0"), (tris["e0"], e0, "e0"), (tris["e1"], e1, "e1")):
        assert np.array_equal(bits(got), bits(want)), what
    assert np.array_equal(tris["model"], lm)
    assert np.array_equal(tris["cull"], np.isin(lm, list(cull)).astype(np.int32))
    leaf_lo, leaf_hi = w.min(1), w.max(1)
    lo = np.stack([nodes["lo_l"], np.stack([nodes["rx0"], nodes["ry0"], nodes["rz0"]], -1)], 1)  # [node, side, 3]
    hi = np.stack([nodes["hi_l"], nodes["hi_r"]], 1)
    link = np.stack([nodes["left"], nodes["right"]], 1)
    for s in (0, 1):
        leaf = link[:, s] < 0
        assert np.array_equal(lo[leaf, s], leaf_lo[~link[leaf, s]]), "a leaf-side box is not its triangle's bounds"
        assert np.array_equal(hi[leaf, s], leaf_hi[~link[leaf, s]]), "a leaf-side box is not its triangle's bounds"
        c = link[~leaf, s]
        assert np.array_equal(lo[~leaf, s], lo[c].min(1)), "an inner-side box is not the union of the child's boxes"
        assert np.array_equal(hi[~leaf, s], hi[c].max(1)), "an inner-side box is not the union of the child's boxes"


def assert_identity(r, models):
    """Criterion 1: every model's own positions again."""
    n0, t0, _ = r.read_bvh()
    for k, (v, _) in enumerate(models):
        r.update_model(k, v)
    n1, t1, _ = r.read_bvh()
    assert n0.tobytes() == n1.tobytes(), "the node bytes changed"
    worst = 0
    finite = np.isfinite(t0["eps"]) & np.isfinite(t1["eps"])
    assert np.array_equal(np.isfinite(t0["eps"]), np.isfinite(t1["eps"]))
    if finite.any():
        worst = int(T.ulps(t0["eps"][finite], t1["eps"][finite]).max())
    print("identity: largest eps difference %d ulp over %d triangles" % (worst, len(t0)))
    assert worst <= 1
    a, b = t0.copy(), t1.copy()
    a["eps"] = b["eps"] = 0
    assert a.tobytes() == b.tobytes(), "the triangle bytes changed"


def tree_case(name):
    """Criteria 1 and 2 for one mesh (one placed instance), whichever builder
    the process uses: identity, then each deformation applied by refit."""
    v, t = MESHES[name]
    r = context([(v, t)], [PLACED])
    before = topology(r)
    assert_exact_tree(r, [(v, t)], [PLACED])  # (the build's boxes are exact bounds too: identity can be bytewise)
    assert_identity(r, [(v, t)])
    for kind in KINDS + ["identity"]:
        d = deformed(name, kind)
        r.update_model(0, d)
        same_topology(before, topology(r))
        assert_exact_tree(r, [(d, t)], [PLACED])


def two_models():
    return [M.icosphere(2), M.wavy_icosphere(2)]


def two_deformed(kind):
    v, _ = M.wavy_icosphere(2)
    if kind == "hostile":
        return v[np.random.default_rng(11).permutation(len(v))].copy()
    return M.wavy_icosphere(2, amp=0.13, freq=4.0)[0]


# ------------------------------------------------------------------- CPU
def make_nodes(links):
    nodes = np.zeros(len(links), rt0.Renderer.BVH_NODE)
    nodes["left"] = [a for a, _ in links]
    nodes["right"] = [b for _, b in links]
    return nodes


def check_order(links, n_tris):
    order, group, parent, height = rt0.bvh_height_order(make_nodes(links), n_tris)
    n = len(links)
    assert sorted(order.tolist()) == list(range(n))
    want_parent = [-1] * n
    for i, (a, b) in enumerate(links):
        for c in (a, b):
            if c >= 0:
                want_parent[c] = i
    assert parent.tolist() == want_parent

    want = [None] * n
    while None in want:  # (no recursion: a chain is n deep)
        for i, pair in enumerate(links):
            kids = [want[c] for c in pair if c >= 0]
            if want[i] is None and None not in kids:
                want[i] = max([0] + [1 + k for k in kids])
    assert height.tolist() == want
    assert group[0] == 0 and group[-1] == n and (np.diff(group) > 0).all() and len(group) == height.max() + 2
    for g in range(len(group) - 1):
        members = order[group[g]:group[g + 1]]
        assert (height[members] == g).all() and (np.diff(members) > 0).all()
    return order, group, height


def test_height_order_small_trees():
    """One triangle (the root holds the leaf twice), one inner node, a chain,
    a full tree, and a renumbered tree (the treelet order moves nodes)."""
    check_order([(~0, ~0)], 1)
    check_order([(~0, ~1)], 2)
    _, group, height = check_order([(~0, 1), (~1, 2), (~2, 3), (~3, ~4)], 5)  # a chain: one node per height
    assert height.tolist() == [3, 2, 1, 0] and group.tolist() == [0, 1, 2, 3, 4]
    _, group, _ = check_order([(1, 2), (3, 4), (5, 6), (~0, ~1), (~2, ~3), (~4, ~5), (~6, ~7)], 8)
    assert group.tolist() == [0, 4, 6, 7]
    # the same tree numbered another way, a leaf next to an inner child
    check_order([(3, ~0), (~1, ~2), (~3, ~4), (2, 1)], 5)


def test_height_order_random_trees():
    rng = np.random.default_rng(5)
    for n_tris in (3, 7, 64, 1000):
        # a random binary tree over the leaves in random order, nodes numbered at random (root 0)
        items = [~int(i) for i in rng.permutation(n_tris)]
        links, free = {}, list(rng.permutation(np.arange(1, n_tris - 1)))
        while len(items) > 1:
            i, j = sorted(rng.choice(len(items), 2, replace=False))
            b, a = items.pop(j), items.pop(i)
            node = int(free.pop()) if len(items) > 0 else 0
            links[node] = (a, b)
            items.append(node)
        check_order([links[i] for i in range(n_tris - 1)], n_tris)


@pytest.mark.parametrize("links,n_tris", [
    ([(~0, ~2)], 2),                       # a leaf out of range
    ([(~0, ~0)], 2),                       # a leaf twice, another never
    ([(~0, ~1)], 1),                       # one triangle: the root must hold it twice
    ([(1, 5), (~0, ~1), (~2, ~3)], 4),     # an inner link out of range
    ([(1, 1), (~0, ~1), (~2, ~3)], 4),     # a node with two parents, another unreachable
    ([(~0, ~1), (2, ~2), (1, ~3)], 4),     # a cycle the root never reaches
    ([(0, ~0), (~1, ~2)], 3),              # the root as a child
])
def test_height_order_rejects_what_is_not_a_tree(links, n_tris):
    with pytest.raises(rt0.Rt0Error) as e:
        rt0.bvh_height_order(make_nodes(links), n_tris)
    assert e.value.code == -1
    assert rt0.lib().rt0_bvh_height_order(None, 4, None, None, None, None, None) == -1
    assert rt0.lib().rt0_bvh_height_order(make_nodes(links).ctypes.data_as(ctypes.c_void_p), 0, None, None, None,
                                          None, None) == -1


# ------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_refit_is_exact_tree(name, gpu_required):
    """Criteria 1 and 2 on the host builder's (binned-SAH) tree, every mesh.

    Measured on the MI355X: the identity refit rewrites the node bytes and the
    triangle bytes exactly; the largest `eps` difference, printed per mesh,
    is 0 ulp (2 ulp on cube_degenerate while the refit still used k_pack's
    FMA-contracted expression on the host builder's tree)."""
    tree_case(name)


@pytest.mark.gpu
def test_refit_two_models_one_updated(gpu_required):
    """Two instances at different pos / joker.x, one with the cull bit; only
    model 1 is updated."""
    models = two_models()
    r = context(models, TWO, cull=(1,))
    before = topology(r)
    assert_exact_tree(r, models, TWO, cull=(1,))
    assert_identity(r, models)
    for kind in KINDS:
        now = [models[0], (two_deformed(kind), models[1][1])]
        r.update_model(1, now[1][0])
        same_topology(before, topology(r))
        assert_exact_tree(r, now, TWO, cull=(1,))


_CHILD = r"""
import sys, traceback, json
sys.path[:0] = sys.argv[1:3]
import test_refit as R
out = {}
for name in ("cube", "wavy3"):
    try:
        R.tree_case(name)
        assert R.context([R.MESHES[name]], [R.PLACED]).read_bvh()[2] == 0  # (the device build numbers no treelet)
        out[name] = ""
    except Exception:
        out[name] = traceback.format_exc()
json.dump(out, open(sys.argv[3], "w"))
"""


@pytest.mark.gpu
def test_refit_is_exact_tree_lbvh(gpu_required, tmp_path):
    """Criteria 1 and 2 on the device LBVH (RT0_BVH_BUILD=lbvh is read at
    process start: a fresh child process), cube and the 1280-triangle sphere."""
    import json
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    out = tmp_path / "lbvh.json"
    env = dict(os.environ, RT0_BVH_BUILD="lbvh", PYTHONPATH=here)
    p = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(repo, "raytracer-0_amd"),
                        os.path.join(repo, "oracle"), str(out)], env=env, timeout=300, capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stderr[-4000:]
    res = json.load(open(out))
    assert res == {"cube": "", "wavy3": ""}, "\n".join(res.values())


def family_rays(soup, case_id, fam):
    rng = np.random.default_rng([case_id, T.FAMILIES.index(fam), 2025])
    o, d, tm = T._GEN[fam](soup, rng, N_RAYS)
    tm = np.full(N_RAYS, T.INF_T) if tm is None else tm
    return (np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32), np.ascontiguousarray(tm, F32))


def walk_vs_loop(r, o, d, tm):
    """test_trace.walk_against_loop on a given context and rays."""
    t0, k0 = r.trace_rays(o, d, tm, 0)
    t1, k1 = r.trace_rays(o, d, tm, 1)
    t2, k2 = r.trace_rays(o, d, tm, 2)
    lost = (k0 < 0) & (k2 >= 0)
    extra = (k0 >= 0) & (k2 < 0)
    both = (k0 >= 0) & (k2 >= 0)
    t_diff = both & (bits(t0) != bits(t2))
    other = both & (k0 != k2) & ~t_diff
    tris = r.read_bvh()[1]
    untied = 0
    for i in np.flatnonzero(other):
        pair = [k0[i], k2[i]]
        ts = []
        for k in pair:  # (each with its own cull bit)
            R = T.tri_test_np(tris["v0"][[k]], tris["e0"][[k]], tris["e1"][[k]], bool(tris["cull"][k]), o[i:i + 1],
                              d[i:i + 1], tm[i:i + 1], np.float64)
            ts.append(R["t"][0, 0])
        untied += not abs(ts[0] - ts[1]) <= T.T_TOL * abs(ts[1])
    occl = (k1 >= 0) != (k2 >= 0)
    return dict(lost=int(lost.sum()), extra=int(extra.sum()), t_diff=int(t_diff.sum()), untied=int(untied),
                occl=int(occl.sum()), hits=int((k2 >= 0).sum())), t0, k0


def ray_case(name, kind, cull):
    """A refitted context and a freshly built one for the deformed mesh."""
    if name == "two":
        models, insts, cl = two_models(), TWO, ((1,) if cull else ())
        now = [models[0], (two_deformed(kind), models[1][1])]
        upd = 1
    else:
        models, insts, cl = [MESHES[name]], [UNIT], ((0,) if cull else ())
        now = [(deformed(name, kind), models[0][1])]
        upd = 0
    r = context(models, insts, cl)
    r.model_info()                       # the tree of the undeformed model
    r.update_model(upd, now[upd][0])     # refit
    fresh = context(now, insts, cl)      # the parent's route: a build from the deformed positions
    soup = np.concatenate([world(v, i)[np.asarray(t)] for (v, t), i in zip(now, insts)])
    return r, fresh, soup


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES + ["two"])
def test_walk_on_refitted_tree(name, kind, cull, gpu_required):
    """Criteria 3 and 4: 4096 rays per family drawn against the deformed soup.

    On the refitted tree the closest-hit walk returns the loop's t bit for
    bit (another triangle only at a float64 tie), loses and adds no hit, and
    the occlusion walk agrees with the loop; and mode-0 t equals, bit for
    bit, that of a context built from the deformed model by set_model.  A
    hit / miss disagreement between the two contexts could only come from a
    differing `eps` (host vs device arithmetic) on a near-parallel triangle:
    the count is printed, expected 0, and capped at 0."""
    r, fresh, soup = ray_case(name, kind, cull)
    case_id = (NAMES + ["two"]).index(name) * 4 + KINDS.index(kind) * 2 + int(cull)
    disagree = 0
    for fam in T.FAMILIES:
        o, d, tm = family_rays(soup, case_id, fam)
        c, t_a, k_a = walk_vs_loop(r, o, d, tm)
        print("refit %-16s %-8s %-8s cull=%d: %s" % (name, kind, fam, cull, c))
        assert c["lost"] == 0 and c["extra"] == 0, (name, kind, fam, cull, c)
        assert c["t_diff"] == 0 and c["untied"] == 0, (name, kind, fam, cull, c)
        assert c["occl"] == 0, (name, kind, fam, cull, c)
        c2, t_b, k_b = walk_vs_loop(fresh, o, d, tm)
        assert c2["lost"] == 0 and c2["extra"] == 0 and c2["t_diff"] == 0 and c2["untied"] == 0 and c2["occl"] == 0
        hm = (k_a >= 0) != (k_b >= 0)
        disagree += int(hm.sum())
        t_differs = ~hm & (bits(t_a) != bits(t_b))
        assert not t_differs.any(), (name, kind, fam, cull, int(t_differs.sum()))
    print("refit %-16s %-8s cull=%d: hit/miss disagreements with a fresh build: %d" % (name, kind, cull, disagree))
    assert disagree == 0


@pytest.mark.gpu
def test_update_from_device_tensor(gpu_required):
    """Criterion 5: a torch tensor on the context's GPU gives the bytes the
    equal numpy array gives, and a later rebuild (set_scene marks the tree
    dirty) builds from the new positions: the lazily fetched host copy."""
    import torch
    v, t = MESHES["wavy3"]
    d = deformed("wavy3", "smooth")
    a = context([(v, t)], [PLACED])
    b = context([(v, t)], [PLACED])
    before = topology(b)
    a.model_info(), b.model_info()
    a.update_model(0, d)
    scale = torch.tensor(2.0, device="cuda:0")
    dev = (torch.from_numpy(d).to("cuda:0") * scale) / scale  # produced on torch's stream, exact
    b.update_model(0, dev)
    del dev
    na, ta, _ = a.read_bvh()
    nb, tb, _ = b.read_bvh()
    assert na.tobytes() == nb.tobytes() and ta.tobytes() == tb.tobytes()
    same_topology(before, topology(b))
    assert_exact_tree(b, [(d, t)], [PLACED])
    # a CPU tensor goes the host way
    a.update_model(0, torch.from_numpy(v))
    assert_exact_tree(a, [(v, t)], [PLACED])
    # rebuild from the positions that only the device held
    meshes, ne, ns, lights = b.get_scene()
    b.set_scene(meshes, ne, ns, len(meshes) - ne - ns, lights)
    assert b.model_info()[0] == len(t)
    assert_exact_tree(b, [(d, t)], [PLACED])
    # a dirty tree: the device positions are stored at once
    b.set_scene(meshes, ne, ns, len(meshes) - ne - ns, lights)
    b.update_model(0, torch.from_numpy(v).to("cuda:0"))
    assert_exact_tree(b, [(v, t)], [PLACED])
    with pytest.raises(ValueError):
        b.update_model(0, torch.from_numpy(v).to("cuda:0").double())


def oracle_with(cfg, cfgs, models, w, h):
    """test_models.oracle_for with the models given as arrays."""
    o = O.Oracle(cfg, cfgs, width=w, height=h)
    meshes, ne, ns, _ = rt0.parse_scene(*rt0.scene_strings(cfg, cfgs))
    vs, owners = [], []
    for k, ((v, t), m) in enumerate(zip(models, meshes[ne + ns:])):
        tri = M.world_triangles(v, t, list(m.pos), m.joker[0])
        vs.append(tri)
        owners.append(np.full(len(tri), k, np.int32))
    o.set_triangles(np.concatenate(vs), np.concatenate(owners))
    return o


@pytest.fixture(scope="module")
def deformed_oracle_frames(cfgs):
    cfg = TM.cfg_by_name(cfgs, "tri_models")
    models = TM.model_data(cfg)
    models[1] = (M.wavy_icosphere(3, amp=0.15, freq=4.0)[0], models[1][1])
    o = oracle_with(cfg, cfgs, models, 64, 64)
    return models, [o.frame(k)[0] for k in (1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [True, False])
def test_rendered_image_after_refit(cfgs, gpu_required, jit, deformed_oracle_frames):
    """Criterion 6: tri_models at 64x64; render, update_model(1, deformed),
    clear, passes 1 and 2 against the brute-force oracle of the deformed
    model (test_models_match_bruteforce_oracle's criteria), on the same
    render path and without a hipRTC compilation."""
    cfg = TM.cfg_by_name(cfgs, "tri_models")
    models, frames = deformed_oracle_frames
    r = TM.make(cfg, cfgs, 64, 64, jit)
    r.render(1, 1)
    path, compiles, info = r.last_render_path(), rt0.jit_compiles(), r.model_info()
    first = r.read_accum()
    r.update_model(1, models[1][0])
    for k, ref in zip((1, 2), frames):
        r.clear()
        r.render(k, 1)
        got = r.read_accum()
        ok = TM.pixel_match(got[..., :3], ref[..., :3])
        assert ok.mean() >= 0.98, (k, ok.mean())
        assert abs(got[..., :3].mean() - ref[..., :3].mean()) <= 5e-3 * max(1.0, ref[..., :3].mean())
        if k == 1:
            assert not np.array_equal(got, first)
    assert r.last_render_path() == path
    assert rt0.jit_compiles() == compiles, "the refit recompiled the scene's kernel"
    assert r.model_info() == info


@pytest.mark.gpu
def test_update_model_errors_and_stores(gpu_required):
    """Criterion 7."""
    v, t = MESHES["cube"]
    d = deformed("cube", "smooth")
    r = rt0.Renderer(16, 16)
    r.set_model(0, v, t)
    with pytest.raises(rt0.Rt0Error) as e:  # no scene yet
        r.update_model(0, v)
    assert e.value.code == -4
    r.set_scene_glsl(rt0.scene_from_lines(scene_lines([PLACED]))[0])
    for k, pos in ((0, v[:-1]), (0, np.concatenate([v, v])), (1, v), (5, v), (-1, v)):
        with pytest.raises(rt0.Rt0Error) as e:
            r.update_model(k, pos)
        assert e.value.code == -1, (k, len(pos))
    # a dirty (never built) tree: the positions are stored, the next build has them
    r.update_model(0, d)
    assert r.model_info()[0] == len(t)
    assert_exact_tree(r, [(d, t)], [PLACED])
    with pytest.raises(rt0.Rt0Error) as e:
        r.update_model(0, v[:-1])
    assert e.value.code == -1
    # joker.x == 0: the instance has no leaves, the update leaves the device arrays alone
    models = two_models()
    z = context(models, [TWO[0], (TWO[1][0], 0.0)])
    assert z.model_info()[0] == len(models[0][1])
    n0, t0, _ = z.read_bvh()
    z.update_model(1, two_deformed("hostile"))
    n1, t1, _ = z.read_bvh()
    assert n0.tobytes() == n1.tobytes() and t0.tobytes() == t1.tobytes()
    assert (z.leaf_source()[0] == 0).all()
    # ... and a model without triangles
    e0 = context([(v, t), (v, np.zeros((0, 3), np.int32))], TWO)
    n0, t0, _ = e0.read_bvh()
    e0.update_model(1, d)
    n1, t1, _ = e0.read_bvh()
    assert n0.tobytes() == n1.tobytes() and t0.tobytes() == t1.tobytes()

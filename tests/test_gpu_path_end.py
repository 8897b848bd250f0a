"""Deferred path end (RT0_PATH_END_DEFER, rt0_integrator.h path_end): the
plain pass kernel evaluates a path's light hit once per sample, where the wave
has reconverged, instead of inside the bounce loop.  Same inputs, same
arithmetic, same order: every accumulator must equal, bit for bit, the one the
inline form produces (RT0_JIT_EXTRA=-DRT0_PATH_END_DEFER=0, the same module
with the define off), and instantiations outside the scope must not notice
the define at all."""
import numpy as np
import pytest

import rt0
from test_gpu_parity import cfg_by_name, configure

pytestmark = pytest.mark.gpu

INLINE = "-DRT0_PATH_END_DEFER=0"
DEFER = "-DRT0_PATH_END_DEFER=1"


def variant(monkeypatch, extra):
    if extra:
        monkeypatch.setenv("RT0_JIT_EXTRA", extra)
    else:
        monkeypatch.delenv("RT0_JIT_EXTRA", raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def renders(cfgs, name, w, h, setup=None):
    """Accumulators after passes 1..1, 1..3, 1..64 (each from a cleared
    buffer) and after a second call that continues the last one at pass 65."""
    r = rt0.Renderer(w, h)
    configure(r, cfg_by_name(cfgs, name), cfgs)
    if setup:
        setup(r)
    out = []
    for frames in (1, 3, 64):
        r.clear()
        r.render(1, frames)
        out.append(r.read_accum())
    r.render(65, 3)
    out.append(r.read_accum())
    r.close()
    return out


# the light seen from the camera (depth 0, w = 1) and MIS-weighted deeper hits;
# MIS off; sample_lights off (every hit w = 1); a specular bounce before the
# light and a non-zero aperture.  16x16 is one tile, 40x24 has partial tiles
# (lanes that return before the loop).
@pytest.mark.parametrize("size", [(16, 16), (40, 24)])
@pytest.mark.parametrize("name", ["c2_cornell_mis_8", "cornell_nee_plain", "c1_cornell_cos", "thinlens_glass"])
def test_path_end_defer_is_bit_identical(name, size, cfgs, monkeypatch, gpu_required):
    variant(monkeypatch, INLINE)
    ref = renders(cfgs, name, *size)
    variant(monkeypatch, None)  # the default build
    got = renders(cfgs, name, *size)
    for what, a, b in zip(("1 pass", "3 passes", "64 passes", "64 + 3 passes"), ref, got):
        assert np.array_equal(bits(a), bits(b)), what
    assert np.isfinite(got[3]).all() and got[2][..., :3].mean() > 0.0


def test_path_end_defer_band_shard_compact(cfgs, monkeypatch, gpu_required):
    """One band shard rendering into a band-packed accumulator."""
    import torch
    W, H = 40, 48
    out = []
    for extra in (INLINE, None):
        variant(monkeypatch, extra)
        buf = torch.zeros((32, W, 4), dtype=torch.float32, device="cuda:0")

        def setup(r):
            r.set_shard(0, 2, 16)
            assert r.set_accum_buffer_compact(buf.data_ptr()) == 32

        out.append(renders(cfgs, "c2_cornell_mis_8", W, H, setup))
        del buf
    for a, b in zip(*out):  # (read_accum fills the packed rows only)
        assert np.array_equal(bits(a[:32]), bits(b[:32]))
    assert np.isfinite(out[1][3][:32]).all() and out[1][2][:32, :, :3].mean() > 0.0


def test_path_end_defer_register_path_matches_frame_chunks(cfgs, monkeypatch, gpu_required):
    """A small launch of several passes is frame-chunked (samples through
    Integrator::sample, summed by rt0_sum_kernel); one pass per launch keeps
    the accumulator in registers (pixel_passes).  Both call path_end: the two
    agree with each other and with the inline form."""
    out = {}
    for extra in (INLINE, None):
        variant(monkeypatch, extra)
        r = rt0.Renderer(40, 24)
        configure(r, cfg_by_name(cfgs, "c2_cornell_mis_8"), cfgs)
        r.render(1, 5)
        chunked = r.read_accum()
        r.clear()
        for k in range(1, 6):
            r.render(k, 1)
        out[extra] = (chunked, r.read_accum())
        r.close()
    assert np.array_equal(bits(out[None][0]), bits(out[None][1]))
    assert np.array_equal(bits(out[None][0]), bits(out[INLINE][0]))
    assert np.array_equal(bits(out[None][1]), bits(out[INLINE][1]))


def test_path_end_defer_multi_pass_register_loop(cfgs, monkeypatch, gpu_required):
    """Several passes in one unchunked launch -- pixel_passes' frame loop, which
    the host takes from 1024^2 pixels on (the bench shape): passes 1..3, then
    resumed at 4."""
    out = []
    for extra in (INLINE, None):
        variant(monkeypatch, extra)
        r = rt0.Renderer(1024, 1024)
        configure(r, cfg_by_name(cfgs, "c2_cornell_mis_8"), cfgs)
        r.render(1, 3)
        a = r.read_accum()
        r.render(4, 2)
        out.append((a, r.read_accum()))
        r.close()
    for a, b in zip(*out):
        assert np.array_equal(bits(a), bits(b))


def scope_c3(cfgs):
    r = rt0.Renderer(40, 24)
    cfg = cfg_by_name(cfgs, "c3_outdoor_restir")
    configure(r, cfg, cfgs)
    r.set_temporal_frames(cfg.get("temporal_frames", 5))
    return r


def scope_quad(cfgs):
    r = rt0.Renderer(40, 24)
    configure(r, cfg_by_name(cfgs, "spectral_2l_novol"), cfgs)
    r.set_executor_compat(True)  # the quad-shared light index: quad_rec()
    return r


def scope_tex(cfgs):
    r = rt0.Renderer(40, 24)
    configure(r, cfg_by_name(cfgs, "tex_light_sphere"), cfgs)  # the light's colour is a texel at the hit
    return r


def scope_sdf(cfgs):
    r = rt0.Renderer(40, 24)
    configure(r, cfg_by_name(cfgs, "mis_demo_sdfbox"), cfgs)  # wavefront rounds (WF)
    return r


@pytest.mark.parametrize("make", [scope_c3, scope_quad, scope_tex, scope_sdf])
def test_path_end_defer_scope(make, cfgs, monkeypatch, gpu_required):
    """ReSTIR, executor-compat (quad record), textured and SDF instantiations
    keep the inline form whatever the define says."""
    out = []
    for extra in (INLINE, DEFER):
        variant(monkeypatch, extra)
        r = make(cfgs)
        acc = []
        for k in range(1, 4):
            r.render(k, 1)
            acc.append(r.read_accum())
        r.clear()
        r.render(1, 3)
        acc.append(r.read_accum())
        r.close()
        out.append(acc)
    for a, b in zip(*out):
        assert np.array_equal(bits(a), bits(b))
    assert np.isfinite(out[1][-1]).all() and out[1][-1][..., :3].mean() > 0.0

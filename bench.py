#!/usr/bin/env python3
"""bench.py -- Msamples/s of the rt0 HIP integrator on BASELINE.json's workloads.

Default workload (BASELINE.json configs[1], SURVEY 8d "C2"): 1024x1024 Cornell
box (index.js:54-85, camera index.js:89-95), MIS power heuristic on, 8 bounces
(MAX_BOUNCES = MAX_DIFF_BOUNCES = 8: a true 8-bounce path; the reference's
default MAX_DIFF_BOUNCES=4 variant is reported beside it with --secondary),
64 spp.  One step = one 64-pass progressive render of the whole image
(u_frame 1..64, i.e. 64 GlslViewport.render() calls) with scene + accumulator
resident in HBM.  `--config c1|c3|c4|c5` times the other BASELINE configs
(rt0/workloads.json); C3/C5 are ReSTIR workloads whose steps continue the
frame sequence (temporal reuse needs u_frame > 2).

N GPUs: `python bench.py --gpus N` starts `torch.distributed.run` with N
ranks as a child process (before anything touches a GPU) unless it already
runs under it; WORLD_SIZE must equal --gpus.  One process per GPU:
  * progressive workloads (C1, C2, C4): the image is split into 16-row bands
    dealt round-robin over ranks (rt0_set_shard); each rank renders its bands
    straight into a band-packed torch buffer (rt0_set_accum_buffer_compact:
    the RCCL send buffer as it stands), and rank 0 gathers the bands over RCCL
    into one preallocated buffer and reorders them with one index_copy_.
    Each workload names its scaling (workloads.json): C1/C2 "strong" -- a
    step is the N = 1 job split N ways (C2: BASELINE's fixed 1024^2 x 64 spp);
    C4 "weak" -- a step at N GPUs renders N x spp passes, every rank its 1/N
    of the rows for all of them (C4 at N = 8 is the 64-spp render BASELINE.md
    quotes).  At N > 1 the other mode's job is timed after the primary one and
    reported as secondary_<mode>_Msamples_s (config.job / secondary_job say
    which job each number is); `--scaling` overrides the primary mode;
  * ReSTIR workloads (C3, C5): two round-robin row bands per rank
    (shard.interleaved_band), a halo exchange of the newest reservoir planes
    at every band boundary after every pass (RCCL point-to-point,
    rt0/shard.py: RestirShard), the band gather at the end of the step.
librt0 launches on its own stream; it is ordered against torch's stream (the
accumulator zeroing, the exchanges, the gather) with events, so steps run back
to back with no host synchronisation between them (one device-wide
synchronize ends the timed region; the last step's kernel time is read
after it).  Both gathers are inside the timed
region; rank 0's gather time is reported
separately.  `--dist-backend gloo` stages every transfer through host memory:
the one-GPU rehearsal of the N>1 path (all ranks on one device with
RT0_BENCH_DEVICE=0, tests/test_bench_dist.py).

A plain run (`bench.py --gpus N --steps K --warmup W`) does only what the
headline figure needs: set-up, W warm-up steps, K timed steps, the outputs
(`--dump-outputs DIR`: the HDR image of the last timed step as DIR/image.npy,
float32; an image over 48 MB as a fixed, seeded sample of its pixels) and ONE
JSON line on rank 0 with `value` and `ms_per_step`.  Everything else runs
only with `--full`: at N > 1 the other scaling mode's job, the GPU clock
sampled during the timed region, the secondary line (c2, c4), and
`roofline` (VALU FP32: algorithmic FLOP/sample from SURVEY 8d x counted events,
over the kernel's HIP-event time; HBM traffic from the committed PMC passes)
and, at N=1, `cpu_baseline` (the JS CPU integrator
raytracer-0_amd/js/rt0_cpu.js on node worker_threads, bounded sample of the same
workload) with the C restatement oracle/rt0_oracle.c (OpenMP) beside it as
`cpu_baseline_c`.  Only those two baseline legs touch oracle/.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "raytracer-0_amd"))

PEAK_FP32_TFLOPS = 157.3  # MI355X vector FP32 (MI355X_MICROARCH.md, chip table)
PEAK_HBM_GBS = 8000.0
# profiles/<dir>/ holding the PMC summaries (pmc_<config>.json) of each
# workload, newest first (scripts/gpu_measure.sh writes them)
PROFILE_ROUNDS = ("r06", "r05", "r04", "r03", "r02/final")
BAND = 16


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def relaunch(n):
    """Run this script under torch.distributed.run with n ranks (a child
    process: nothing here has touched the GPU) and return its exit code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


# ---------------------------------------------------------------- FLOP model
def isect_flop(scene):
    """SURVEY 8d per-intersection() weights counted from source: iPlane 12,
    iSphere 20, iBox 23 FLOP per candidate (raytracer.glsl:812-859), plus ~25
    for the closest-hit parse (1049-1079).  Cornell (5 planes, 1 sphere,
    2 boxes) = 151, the 150 of SURVEY 8d."""
    n = {"PLANE": 0, "SPHERE": 0, "BOX": 0}
    for line in scene:
        t = [x.strip() for x in line.split(",")]
        if len(t) > 1 and t[1] in n:
            n[t[1]] += 1
    return 12.0 * n["PLANE"] + 20.0 * n["SPHERE"] + 23.0 * n["BOX"] + 25.0


# FLOP of one map() evaluation per SDF kind (raytracer.glsl:496-712, counted
# from source as in SURVEY 8d): sdBox 0, udRoundBox 1, sdSphere 2,
# sdTriPrism 3, sdCone 4, Menger 5, Mandelbulb 6 (index.html:702-717); + 4 for
# the p - pos offset and the min() of map().
MAP_FLOP = {0: 17.0, 1: 16.0, 2: 8.0, 3: 18.0, 4: 16.0, 5: 140.0, 6: 190.0}


# Terms the SURVEY 8d formula leaves out, counted from source the same way
# (per event, events counted by the counting instance, rt0_read_counters_n):
#  - ReSTIR (raytracer.glsl:1619-1801): per sampleLightsReSTIR call the
#    finalize + weight arithmetic (1525-1576, 1759-1795) 90; per candidate
#    (hash2, light pick, evaluateTargetFunction 1361-1387, updateReservoir)
#    80; per temporal tap (hash2 jitter, two bilinear RGBA32F fetches, unpack
#    1437-1468, isValidReservoir, decay, combineReservoirs 1579-1611) 210; per
#    spatial tap (the same without the motion/decay terms) 180.  The
#    visibility ray is already an intersection() and the final
#    calcDirectLighting a NEE call.
#  - triangle models (no reference code): per BVH node visited two slab tests
#    50, per Moller-Trumbore test (raytracer.glsl:864-892, commented out) 45.
RESTIR_FLOP = {"restir": 90.0, "restir_cand": 80.0, "restir_ttap": 210.0, "restir_stap": 180.0}
BVH_FLOP = {"bvh_node": 50.0, "tri": 45.0}


def flop_per_sample(c, wl):
    """SURVEY 8d algorithmic FLOP model, per sample:
    140 + C_isect*isect + 130*iter + (140 + 54*mis)*nee + C_map*map,
    plus the ReSTIR and BVH terms above."""
    n = max(1, c["samples"])
    mis = bool(wl["constants"].get("use_mis", False))
    c_map = sum(MAP_FLOP[k] for k in wl.get("sdf_kinds", [])) or 0.0
    extra = sum(w * c.get(k, 0) for k, w in list(RESTIR_FLOP.items()) + list(BVH_FLOP.items())) / n
    return (140.0 + isect_flop(wl["scene_lines"]) * c["isect"] / n + 130.0 * c["iter"] / n
            + (140.0 + 54.0 * mis) * c["nee"] / n + c_map * c["map"] / n + extra)


def host_threads():
    """Host threads the baselines may use: OMP_NUM_THREADS (16 on the GPU box,
    whose os.cpu_count() shows the whole machine), else up to 16."""
    return int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1)


# ------------------------------------------------------------ CPU baselines
def cpu_baseline_js(wl, budget_s=10.0):
    """SURVEY 8d's CPU baseline: the JS CPU integrator (raytracer-0_amd/js/rt0_cpu.js,
    fp32 restatement of the same integrator, parity-checked in
    tests/test_cpu_js.py) on node worker_threads, timed on a bounded sample of
    the same workload: a 64-row band through the image centre, successive
    passes until the time budget (ReSTIR workloads: the band's passes run
    the reservoir chain, the rest of the planes stays empty).  Workloads with
    triangle models: the JS integrator tests every triangle per ray (like the
    C restatement; the reference has no triangle path), so the sample is a
    16-row x 64-column patch at the image centre."""
    import shutil
    import tempfile
    node = shutil.which("node")
    if node is None:
        return None
    threads = host_threads()
    W, H = wl["width"], wl["height"]
    r0, rows, extra, what = H // 2 - 32, 64, [], ""
    tmp = None
    if wl.get("models"):
        import numpy as np
        sys.path.insert(0, os.path.join(HERE, "oracle"))
        import oracle as O
        from rt0 import meshes, workloads
        inst = workloads.model_instances(wl)
        soup = [meshes.world_triangles(v, t, pos, scale) for v, t, pos, scale, _ in inst]
        owners = np.concatenate([np.full(len(x), i[4], np.int32) for x, i in zip(soup, inst)])
        tmp = tempfile.mkdtemp(prefix="rt0_js_")
        O.write_tris(os.path.join(tmp, "tris.bin"), np.concatenate(soup), owners)
        r0, rows = H // 2 - 8, 16
        x0 = W // 2 - 32
        extra = ["--tris", os.path.join(tmp, "tris.bin"), "--xspan", str(x0), str(x0 + 64)]
        what = ", columns %d..%d, brute force over all %d triangles per ray" % (x0, x0 + 63, len(owners))
    try:
        r = subprocess.run([node, os.path.join(HERE, "oracle", "js", "cpu_bench.js"),
                            os.path.join(HERE, "tests", "golden", "configs.json"), wl["fixture"], str(W), str(H),
                            str(threads), "restir-bench" if wl.get("defines", {}).get("USE_RESTIR") else "bench",
                            str(r0), str(r0 + rows), str(budget_s)]
                           + (["--constants", json.dumps(wl["constants"])]) + extra,
                           capture_output=True, text=True, timeout=budget_s * 10 + 60)
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    if r.returncode != 0:
        return {"error": r.stderr[-300:]}
    d = json.loads(r.stdout)
    return {"value": d["msamples_s"], "unit": "Msamples/s", "cores": d["threads"], "kind": "port",
            "sample": "raytracer-0_amd/js/rt0_cpu.js (JS CPU integrator, node %s worker_threads x%d, %s): rows %d..%d of "
                      "the %dx%d bench image%s, successive passes, %d samples in %.1f s"
                      % (d["node"], d["threads"], d["cpu"], r0, r0 + rows - 1, W, H, what, d["samples"], d["seconds"])}


def cpu_baseline_c(wl, budget_s=8.0):
    """Time the C restatement (OpenMP, all host threads we are allowed) on a
    bounded sample of the same workload: a full-width band of 64 rows through
    the image centre, successive passes, scaled by samples."""
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, "oracle"))
    import oracle as O
    threads = host_threads()
    W, H = wl["width"], wl["height"]
    rows, r0 = 64, H // 2 - 32
    cfg = {"scene_lines": wl["scene_lines"], "sdf_kinds": wl.get("sdf_kinds", []), "defines": wl["defines"],
           "constants": wl["constants"], "camera": wl["camera"], "models": wl.get("models", [])}
    o = O.Oracle(cfg, {"cornell_lines": None, "default_camera": wl["camera"]}, width=W, height=H)
    what = ""
    if wl.get("models"):
        # the restatement (like the reference, which has no triangle path at
        # all) loops over every triangle per ray: a one-row sample, ~5 s a row
        from rt0 import meshes, workloads
        inst = workloads.model_instances(wl)
        soup = [meshes.world_triangles(v, t, pos, scale) for v, t, pos, scale, _ in inst]
        v9 = np.concatenate(soup)
        o.set_triangles(v9, np.concatenate([np.full(len(x), i[4], np.int32) for x, i in zip(soup, inst)]))
        rows, r0 = 1, H // 2
        what = ", brute force over all %d triangles per ray" % len(v9)
    else:
        o.frame(1, rows=(r0, r0 + 8), threads=threads)  # warm
    n = 0
    t0 = time.time()
    while time.time() - t0 < budget_s:
        o.frame(1 + n, rows=(r0, r0 + rows), threads=threads)
        n += 1
    dt = time.time() - t0
    samples = n * rows * W
    return {"value": samples / dt / 1e6, "unit": "Msamples/s", "cores": threads, "kind": "port",
            "sample": "oracle/rt0_oracle.c (OpenMP x%d), rows %d..%d of the %dx%d bench image, %d passes "
                      "(%d samples, %.1f s)%s" % (threads, r0, r0 + rows - 1, W, H, n, samples, dt, what)}


# ------------------------------------------------------------- GPU clock
class ClockSampler:
    """Samples the GPU's current shader clock during the timed region (the C2
    kernel moves 5.26-5.45 ms with the box's clock, DESIGN 5.00, as much as most
    A/B deltas): the starred level of the amdgpu driver's pp_dpm_sclk for the
    device's PCI address, read once right before and once right after the
    timed region and every 25 ms in between by a host thread (no GPU call; a
    sysfs read releases the GIL).  Reports the median and range, or why it
    could not (the file missing or unreadable for this user)."""

    def __init__(self, torch, local):
        import glob
        self.path, self.err, self.mhz = None, None, []
        try:
            props = torch.cuda.get_device_properties(local)
            bus, dom = int(props.pci_bus_id), int(getattr(props, "pci_domain_id", 0))
        except Exception as e:  # noqa: BLE001 -- reported, not fatal
            bus, dom, self.err = None, None, "no pci_bus_id: %s" % e
        if bus is not None:
            # the device directory is named by its PCI address, DDDD:BB:DD.F (hex)
            for cand in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
                addr = os.path.basename(os.path.realpath(os.path.dirname(cand)))
                parts = addr.replace(".", ":").split(":")
                try:
                    if len(parts) == 4 and int(parts[1], 16) == bus and int(parts[0], 16) == dom:
                        self.path = cand
                        break
                except ValueError:
                    continue
            if self.path is None:
                self.err = "no pp_dpm_sclk for PCI %04x:%02x" % (dom, bus)
        self._stop = None
        self._th = None

    def _read(self):
        try:
            for line in open(self.path):
                if line.rstrip().endswith("*"):
                    return float(line.split(":")[1].strip().lower().replace("mhz", "").replace("*", "").strip())
        except (OSError, ValueError, IndexError) as e:
            self.err = "%s: %s" % (self.path, e)
        return None

    def sample(self):
        if self.path is not None:
            v = self._read()
            if v is not None:
                self.mhz.append(v)

    def start(self):
        import threading
        if self.path is None:
            return
        self.sample()
        self._stop = threading.Event()

        def run():
            while not self._stop.wait(0.025):
                self.sample()
        self._th = threading.Thread(target=run, daemon=True)
        self._th.start()

    def stop(self):
        if self._th is not None:
            self._stop.set()
            self._th.join()
        self.sample()

    def report(self):
        if not self.mhz:
            return {"median_mhz": None, "source": self.path, "error": self.err or "no samples"}
        m = sorted(self.mhz)
        return {"median_mhz": m[len(m) // 2], "min_mhz": m[0], "max_mhz": m[-1], "samples": len(m),
                "source": self.path + " (current level: before, every 25 ms during and after the timed region)"}


# ---------------------------------------------------------------- workloads
class Progressive:
    """C1/C2/C4: 16-row bands round-robin, band-packed accumulators, one gather."""

    def __init__(self, rt0, torch, wl, rank, world, local, staged=False, spp=None):
        import rt0.shard as shard
        from rt0 import workloads
        self.torch, self.world = torch, world
        W, H = wl["width"], wl["height"]
        self.r = rt0.Renderer(W, H, device=local)
        workloads.configure(self.r, wl)
        self.spp = spp or wl["spp"]
        self.gather = None
        if world > 1:
            self.r.set_shard(rank, world, BAND)
            self.gather = shard.BandGather(H, W, rank, world, BAND, "cuda:%d" % local, staged=staged)
            self.acc = self.gather.acc
            rows = self.r.set_accum_buffer_compact(self.acc.data_ptr())
            assert rows <= self.acc.shape[0], (rows, self.acc.shape)
            self.samples_per_step = rows * W * self.spp
        else:
            self.acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:%d" % local)
            self.r.set_accum_buffer(self.acc.data_ptr())
            self.samples_per_step = W * H * self.spp
        self.order = shard.StreamOrder(self.r, "cuda:%d" % local)
        self.kernel_ms, self.gather_ms, self.launches = [], [], 0
        self.kernel_estimate = False
        self.image = None

    def step(self, i):
        if self.gather is None:
            # one rank: the zeroing goes straight onto librt0's stream (no
            # cross-stream events: C1's 0.045-ms launches are host-bound)
            with self.torch.cuda.stream(self.order.ext):
                self.acc.zero_()
            self.r.render_async(1, self.spp)
            return
        self.acc.zero_()  # torch's stream
        self.order.rt0_after_torch()
        self.r.render_async(1, self.spp)  # librt0's stream
        self.order.torch_after_rt0()
        if self.gather is not None:
            ev = self.order.begin_timing()
            self.image = self.gather.gather()  # RCCL gather of the HDR bands + one reorder on rank 0
            self.order.end_timing(ev)
        # no host synchronisation: the next step's zero_() and render are
        # stream-ordered after this one, so steps run back to back

    def collect(self):
        """After a device-wide synchronize: the last step's kernel time (librt0's
        timing events of its render call) and gather time."""
        self.r.sync()
        ms, n = self.r.last_kernel_ms()
        self.kernel_ms.append(ms)
        self.launches = n
        if self.gather is not None:
            self.gather_ms.append(self.order.elapsed_ms())

    def final_image(self):
        return self.acc if self.world == 1 else self.image


class Restir:
    """C3/C5: one pass per launch (frame-to-frame reservoir dependency); N>1:
    two or four round-robin row bands per rank (the sky rows of C3/C5 cost a fraction
    of the geometry rows: contiguous blocks left the slowest of 8 ranks at
    2.2-2.3x the mean, scripts/restir_shard_sim.py) + per-pass halo exchange
    at each band boundary + band gather."""

    def __init__(self, rt0, torch, wl, rank, world, local, staged=False):
        import rt0.shard as shard
        from rt0 import workloads
        self.torch, self.world = torch, world
        W, H = wl["width"], wl["height"]
        self.r = rt0.Renderer(W, H, device=local)
        workloads.configure(self.r, wl)
        self.spp = wl["spp"]
        self.sh, self.gather = None, None
        dev = "cuda:%d" % local
        self.order = shard.StreamOrder(self.r, dev)
        if world > 1:
            # four round-robin bands per rank where each stays >= 64 rows (C5 at
            # N=8: the slowest rank 1.48 ms vs 1.82 with two, strong-scaling
            # ceiling 0.60 vs 0.52, profiles/r05/shard_sim), else two
            per = 4 if H >= world * 4 * 64 else 2
            band = shard.interleaved_band(H, world, per_rank=per)
            self.sh = shard.RestirShard(self.r, rank, world, H, W, dev, band=band, staged=staged, order=self.order)
            self.gather = shard.BandGather(H, W, rank, world, band, dev, staged=staged)
            # full-size accumulator padded to whole bands; this rank's bands are
            # packed into the gather's send buffer (one index_select per step,
            # into a preallocated buffer)
            nb = (H + band - 1) // band
            self.acc = torch.zeros((nb * band, W, 4), dtype=torch.float32, device=dev)
            self.r.set_accum_buffer(self.acc.data_ptr())
            own = shard.owned_band_rows(rank, world, band, H)
            rows = [y for lo, _ in own for y in range(lo, lo + band)]
            self.rows = torch.tensor(rows, dtype=torch.long, device=dev)
            # every rank's send buffer has the gather's row count (RCCL needs equal sizes)
            self.send_buf = torch.zeros((self.gather.rows, W, 4), dtype=torch.float32, device=dev)
            self.send = self.send_buf[:len(rows)]
            self.samples_per_step = sum(hi - lo for lo, hi in own) * W * self.spp
        else:
            self.acc = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
            self.r.set_accum_buffer(self.acc.data_ptr())
            self.samples_per_step = W * H * self.spp
        self.kernel_ms, self.gather_ms, self.launches = [], [], 0
        self.kernel_estimate = False
        self.image = None

    def step(self, i):
        first = 1 + i * self.spp
        if self.sh is None:
            self.r.render_async(first, self.spp)  # one call, spp launches on librt0's stream
        else:
            self.sh.render(first, self.spp)  # async passes, halo exchanges event-ordered
            ev = self.order.begin_timing()
            self.torch.index_select(self.acc, 0, self.rows, out=self.send)
            self.image = self.gather.gather(self.send_buf)
            self.order.end_timing(ev)
        # no host synchronisation: the next step's passes follow on the same stream

    def collect(self):
        """After a device-wide synchronize: the last step's kernel time."""
        self.r.sync()
        if self.sh is None:
            ms, n = self.r.last_kernel_ms()  # the render call's spp launches
        else:
            # an ESTIMATE: the last pass's kernel time x spp (the timing events
            # of earlier async passes are overwritten; pass times vary in early
            # frames -- temporal taps from frame 3, halved spatial taps below
            # frame 10 -- so the line labels it, kernel_time_source)
            m, _ = self.r.last_kernel_ms()
            ms, n = m * self.spp, self.spp
            self.kernel_estimate = True
            self.gather_ms.append(self.order.elapsed_ms())
        self.kernel_ms.append(ms)
        self.launches = n

    def final_image(self):
        return self.acc[:self.r.height] if self.world == 1 else self.image


def count_events(rt0, wl, local, first_timed, compat=False):
    """Event counts of the timed workload (separate counting kernel instance, a
    fresh whole-image renderer, outside the timed region).  ReSTIR workloads
    count the frames of the first timed step: the chain is rendered up to it
    uncounted (temporal taps start at frame 3, spatial taps are halved below
    frame 10, raytracer.glsl:1660, 1726), then the step's frames are counted."""
    from rt0 import workloads
    r = rt0.Renderer(wl["width"], wl["height"], device=local)
    workloads.configure(r, wl)
    r.set_executor_compat(compat)
    if workloads.restir(wl):
        if first_timed > 1:
            r.render(1, first_timed - 1)
        r.set_counting(True)
        r.render(first_timed, wl["spp"])
    else:
        r.set_counting(True)
        r.render(1, wl["spp"])
    cnt = r.counters()
    r.close()
    return cnt


def pmc_summary(config):
    """(path, summary) of the newest committed rocprofv3 PMC passes of this
    workload (scripts/gpu_measure.sh -> scripts/pmc_summary.py)."""
    for rd in PROFILE_ROUNDS:
        path = os.path.join(HERE, "profiles", rd, "pmc_%s.json" % config)
        if os.path.exists(path):
            return "profiles/%s/pmc_%s.json" % (rd, config), json.load(open(path))
    return None, None


def calibration():
    """{kernel: true bytes / FETCH_SIZE bytes} of scripts/fetch_calib (16-B/lane
    stream, 64-B gathers, bilinear 2x2 RGBA32F taps), committed under profiles/."""
    for rd in PROFILE_ROUNDS:
        path = os.path.join(HERE, "profiles", rd, "calib.json")
        if os.path.exists(path):
            c = json.load(open(path))
            return {k: v["factor"][-1] for k, v in c.items() if v.get("factor")}, "profiles/%s/calib.json" % rd
    return {}, None


def hbm_traffic(pmc, config, pixels, calib):
    """(estimate, low, high) HBM bytes per launch from the PMC counters.
    FETCH_SIZE under-reports a 16-B/lane stream by 2x but reports a 64-B gather
    at x0.99 and bilinear RGBA32F taps at x0.5 (calib), so the correction is by
    access shape: the accumulator read (16 B/pixel, a stream) at x2; the rest at
    x2 for the progressive workloads (streams only), at the bilinear factor for
    C3 (reservoir taps dominate), at the gather factor for C5 (64-B node,
    48-B triangle and record gathers beside the taps); low/high bound the mix
    at x0.5 .. x2.  WRITE_SIZE is exact for 16-B/lane stores."""
    c = pmc["counters"]
    fetch, write = c["FETCH_SIZE"] * 1024.0, c["WRITE_SIZE"] * 1024.0
    acc = 16.0 * pixels
    rest = max(0.0, fetch - acc / 2.0)
    if config in ("c1", "c2", "c2_refcaps", "c4"):
        est = lo = hi = 2.0 * fetch + write
    else:
        f = calib.get("k_bilin", 0.5) if config == "c3" else calib.get("k_node64", 1.0)
        est = acc + rest * f + write
        lo, hi = acc + 0.5 * rest + write, acc + 2.0 * rest + write
    return est, lo, hi


def valu_rates():
    """(ns per non-transcendental, ns per transcendental) wave64 VALU
    instruction per SIMD, measured by scripts/valu_peak (16 independent chains
    per lane at full occupancy; committed under profiles/), or None."""
    for rd in PROFILE_ROUNDS:
        path = os.path.join(HERE, "profiles", rd, "valu_peak.json")
        if os.path.exists(path):
            r = {}
            for line in open(path):
                if line.startswith("{"):
                    d = json.loads(line)
                    r[d["kernel"]] = d.get("wave_instr_per_simd_per_ns")
            if all(r.get(k) for k in ("v_add_f32", "v_mul_f32", "v_fma_f32", "v_exp_f32")):
                norm = 3.0 / (r["v_add_f32"] + r["v_mul_f32"] + r["v_fma_f32"])
                return norm, 1.0 / r["v_exp_f32"], "profiles/%s/valu_peak.json" % rd
    return None


DUMP_MAX_BYTES = 48 << 20  # of the 64 MB a dump may take


def dump_outputs(path, image):
    """--dump-outputs: the last timed step's HDR image (a device tensor,
    H x W x 4 float32) as path/image.npy.  An image over DUMP_MAX_BYTES is
    written as the same pixels every run: a sorted sample drawn without
    replacement by a generator seeded with 0, N x 4."""
    import numpy as np
    a = np.ascontiguousarray(image.cpu().numpy(), dtype=np.float32)
    if a.nbytes > DUMP_MAX_BYTES:
        px = a.reshape(-1, a.shape[-1])
        n = DUMP_MAX_BYTES // (4 * a.shape[-1])
        a = px[np.sort(np.random.default_rng(0).choice(px.shape[0], size=n, replace=False))]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "image.npy"), a)


def result_line(args, wl, world, weak, value, ms_per_step, job):
    """The result line of a plain run (--full adds its entries to it)."""
    import numpy as np
    from rt0 import workloads
    W, H = wl["width"], wl["height"]
    mdb = wl["constants"].get("MAX_DIFF_BOUNCES", 4)
    out = {
        "metric": "Msamples/sec (pixels x spp / s) at 1024^2 Cornell, 8 bounces" if args.config == "c2"
        else "Msamples/sec (pixels x spp / s), BASELINE workload %s" % args.config,
        "value": round(value, 3),
        "unit": "Msamples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "weak" if weak else "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic (the reference's own scene grammar and materials; no external data)",
        "config": {"workload": "%s (%s): %s" % (args.config, wl["fixture"], wl["doc"]),
                   "width": W, "height": H, "spp": wl["spp"], "max_diff_bounces": mdb,
                   "parallelism": ("row-band x%d (16-row bands)" % world) if not workloads.restir(wl)
                   else ("round-robin row bands x%d + reservoir halo exchange" % world),
                   "dist_backend": args.dist_backend if world > 1 else None,
                   "kernel": "scene-specialised (hipRTC JIT)" if args.jit else "ahead-of-time",
                   "executor_compat": bool(args.executor_compat)},
    }
    if wl.get("baseline_spp") and wl["baseline_spp"] != wl["spp"]:
        out["config"]["spp_note"] = ("BASELINE.md quotes this config at %d spp; one bench step renders %d passes "
                                     "(Msamples/s is per sample either way)" % (wl["baseline_spp"], wl["spp"]))
    out["config"]["job"] = ("%dx%d x %d spp per step over %d GPU(s) (%s scaling: %s)"
                            % (W, H, wl["spp"], world, "weak" if weak else "strong",
                               "per-GPU work of the N = 1 step" if weak else "the N = 1 step's job split N ways"))
    if job.gather_ms:
        out["gather_ms_per_step"] = round(float(np.mean(job.gather_ms)), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="c2", help="workload of rt0/workloads.json: c1 c2 c2_refcaps c3 c4 c5")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline figure does not need: the event "
                         "census and roofline, the GPU clock during the timed region, the secondary line (c2, c4), "
                         "the CPU baselines and, at N > 1, the other scaling mode's job")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0: write the last timed step's HDR image (H x W x 4 float32, what a caller of the "
                         "timed path reads back) as DIR/image.npy; over 48 MB, a fixed seeded sample of its pixels")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--secondary", action="store_true", help="(default now; kept for old command lines)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the secondary line: c2 at MAX_DIFF_BOUNCES=4, c4 at MAX_DIFF_BOUNCES=12")
    ap.add_argument("--jit", type=int, default=1, help="1: scene-specialised kernels (default), 0: ahead-of-time")
    ap.add_argument("--executor-compat", action="store_true",
                    help="rt0_set_executor_compat(1): the reference executor's reservoir stores (ReSTIR workloads)")
    ap.add_argument("--dist-backend", default="nccl", choices=("nccl", "gloo"),
                    help="N>1: nccl = RCCL over xGMI; gloo = every transfer staged through host memory")
    ap.add_argument("--save-image", default=None, help="rank 0: np.save the last step's HDR image (H x W x 4)")
    ap.add_argument("--scaling", default=None, choices=("weak", "strong"),
                    help="progressive workloads (C1, C2, C4) at N GPUs: strong = the N = 1 step's spp passes split "
                         "N ways (the fixed job: C2's 1024^2 x 64 spp of BASELINE's metric); weak = a step renders "
                         "N x spp passes, each rank its 1/N of the rows for all of them (per-GPU work fixed; C4 at "
                         "N = 8 is the 64-spp job BASELINE.md quotes).  Default: the workload's `scaling` "
                         "(workloads.json: C1/C2 strong, C4 weak); at N > 1 the other one is timed after it and "
                         "reported as secondary_<mode>_Msamples_s.  ReSTIR workloads are always strong (each pass "
                         "reads the previous pass's reservoirs).")
    ap.add_argument("--spp", type=int, default=None, help="passes per step at N = 1 (default: the workload's)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    # RT0_BENCH_DEVICE pins every rank to one device (the one-GPU rehearsal)
    local = int(os.environ.get("RT0_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))

    import numpy as np
    import torch
    import rt0
    from rt0 import workloads

    wl = workloads.get(args.config)
    dist = None
    staged = args.dist_backend == "gloo"
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group(args.dist_backend)  # "nccl" = RCCL on ROCm
    W, H = wl["width"], wl["height"]

    base_spp = args.spp or wl["spp"]
    mode = "strong" if workloads.restir(wl) else (args.scaling or wl.get("scaling", "strong"))
    weak = mode == "weak"
    step_spp = base_spp * world if weak else base_spp  # passes per step over the whole image
    wl = dict(wl, spp=step_spp)

    def make_job(w):
        j = (Restir if workloads.restir(w) else Progressive)(rt0, torch, w, rank, world, local, staged=staged)
        j.r.set_jit(bool(args.jit))
        j.r.set_executor_compat(args.executor_compat)
        return j

    def timed(j, clock=None):
        """W untimed steps, then K steps between a barrier + device-wide
        synchronize on both sides; the max over ranks of the timed span."""
        for i in range(args.warmup):
            j.step(i)
        j.kernel_ms.clear()
        j.gather_ms.clear()
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        if clock:
            clock.start()
        t0 = time.perf_counter()
        for i in range(args.steps):
            j.step(args.warmup + i)
        torch.cuda.synchronize()  # device-wide: librt0's stream included
        if dist:
            dist.barrier()
        span = time.perf_counter() - t0
        if clock:
            clock.stop()
        j.collect()  # the last timed step's kernel time, read outside the timed region
        if dist:
            t = torch.tensor([span], device="cuda:%d" % local) if not staged else torch.tensor([span])
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            span = float(t.item())
        return span

    job = make_job(wl)
    clock = ClockSampler(torch, local) if args.full else None
    dt = timed(job, clock)
    # --full, N > 1, progressive: the other scaling mode's job after the primary
    # one, every rank, so a SCALE record holds both the fixed job and the per-GPU one
    second = None
    if args.full and world > 1 and not workloads.restir(wl):
        mode2 = "strong" if weak else "weak"
        wl2 = dict(wl, spp=base_spp * world if mode2 == "weak" else base_spp)
        job2 = make_job(wl2)
        dt2 = timed(job2)
        second = (mode2, wl2, job2, W * H * wl2["spp"] * args.steps / dt2 / 1e6)
    ms_per_step = dt * 1000.0 / args.steps
    total_samples = W * H * wl["spp"] * args.steps  # every rank's share: the whole image
    value = total_samples / dt / 1e6

    if rank != 0:
        dist.destroy_process_group()
        return
    if args.save_image:
        np.save(args.save_image, job.final_image().cpu().numpy()[:H])
        if second:
            root, ext = os.path.splitext(args.save_image)
            np.save(root + "_secondary" + (ext or ".npy"), second[2].final_image().cpu().numpy()[:H])

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, job.final_image()[:H])
    if not args.full:
        print(json.dumps(result_line(args, wl, world, weak, value, ms_per_step, job)), flush=True)
        if dist:
            dist.destroy_process_group()
        return

    first_timed = 1 + args.warmup * wl["spp"]
    cnt = count_events(rt0, wl, local, first_timed, args.executor_compat)
    fps = flop_per_sample(cnt, wl)
    kern_s = float(np.mean(job.kernel_ms)) / 1000.0  # all launches of one step on rank 0
    achieved_tflops = fps * job.samples_per_step / kern_s / 1e12
    per_launch = max(1, job.launches)
    kern_launch_s = kern_s / per_launch
    # algorithmic HBM bytes per launch: one float4 accumulator read +
    # write per pixel (32 B); a ReSTIR pass also writes the two reservoir MRTs
    # and reads the six input planes once (+128 B)
    # (a ReSTIR launch is one pass over the pixels, a progressive launch every
    # pass of the step: either way pixels x bpp)
    bpp = 160.0 if workloads.restir(wl) else 32.0
    alg_bytes = bpp * job.samples_per_step / wl["spp"]
    # HBM traffic per launch from the committed rocprofv3 PMC passes of this
    # workload (FETCH_SIZE x2 gfx950 correction); counters cannot be read from
    # inside this process
    pmc_path, pmc = pmc_summary(args.config) if world == 1 else (None, None)
    calib, calib_src = calibration()
    traffic = lo = hi = None
    if pmc and "FETCH_SIZE" in pmc.get("counters", {}):
        traffic, lo, hi = hbm_traffic(pmc, args.config, W * H, calib)
    roof = {"bound": "valu", "achieved": round(achieved_tflops, 3), "peak": PEAK_FP32_TFLOPS,
            "unit": "TFLOP/s", "frac": round(achieved_tflops / PEAK_FP32_TFLOPS, 4), "traffic": traffic,
            "traffic_range": [lo, hi] if traffic else None, "traffic_calibration": calib_src,
            "traffic_unit": "bytes/launch", "traffic_source": pmc_path,
            "algorithmic_bytes": alg_bytes,
            "algorithmic_gbs": round(alg_bytes / kern_launch_s / 1e9, 1),
            "hbm_gbs": round(traffic / kern_launch_s / 1e9, 1) if traffic else None,
            "hbm_peak_gbs": PEAK_HBM_GBS,
            "hbm_frac": round(traffic / kern_launch_s / 1e9 / PEAK_HBM_GBS, 4) if traffic else None,
            "flop_per_sample": round(fps, 1),
            "events_per_sample": {k: round(cnt[k] / max(1, cnt["samples"]), 3) for k in cnt if k != "samples"},
            "events_window": ("frames %d..%d (the first timed step)" % (first_timed, first_timed + wl["spp"] - 1))
            if workloads.restir(wl) else "frames 1..%d (every step)" % wl["spp"],
            "kernel_ms_per_step": round(kern_s * 1000.0, 3),
            "launches_per_step": job.launches,
            "kernel_ms_per_launch": round(kern_launch_s * 1000.0, 3),
            "kernel_time_source": "ESTIMATE: rank 0's last pass (HIP events) x passes per step"
            if job.kernel_estimate else "HIP events on librt0's stream around the last timed step's launches",
            # counters cannot be read from inside this process: traffic comes
            # from the committed rocprofv3 --pmc passes of the same workload
            "traffic_measured_in_this_run": False,
            "note": "FP32 vector kernel (no MFMA): peak = MI355X FP32 vector 157.3 TF; FLOP model SURVEY 8d x "
                    "counted events (counting instance, whole image); achieved over rank 0's kernel time (HIP "
                    "events on librt0's stream); traffic = PMC FETCH_SIZE corrected per access shape (hbm_traffic) + "
                    "WRITE_SIZE per launch; hbm_gbs = traffic over the same kernel time"}
    if pmc and "valu" in pmc:
        roof["valu_lane_utilisation"] = round(pmc.get("valu_lane_utilisation", 0.0), 4)
        rates = valu_rates()
        if rates:
            # VALU busy: the launch's wave64 VALU instructions at the MEASURED
            # issue time of their class (scripts/valu_peak: add/mul/fma ~0.9-1.1
            # per SIMD per ns, a transcendental ~4.5 ns), over 1024 SIMDs x the
            # live kernel time of one launch
            v = pmc["valu"]
            busy_ns = ((v["SQ_INSTS_VALU"] - v["SQ_INSTS_VALU_TRANS_F32"]) * rates[0]
                       + v["SQ_INSTS_VALU_TRANS_F32"] * rates[1]) / 1024.0
            roof["valu_busy"] = round(busy_ns / (kern_launch_s * 1e9), 4)
            roof["valu_rates_source"] = rates[2]
    out = result_line(args, wl, world, weak, value, ms_per_step, job)
    out["roofline"] = roof
    if second:
        mode2, wl2, _, v2 = second
        out["secondary_%s_Msamples_s" % mode2] = round(v2, 3)
        out["config"]["secondary_job"] = ("%dx%d x %d spp per step over %d GPUs (%s scaling), timed after the "
                                          "primary job with the same steps / warmup"
                                          % (W, H, wl2["spp"], world, mode2))
    out["gpu_clock"] = clock.report()
    if not args.no_secondary and world == 1 and args.config in ("c2", "c4"):
        # after the timed region, same renderer: C2 at the reference's caps
        # (MAX_DIFF_BOUNCES = 4, SURVEY 8d "report both"); C4 at its true depth
        # (MAX_DIFF_BOUNCES = 12: the timed line keeps the reference's 4, a cap
        # the 12-bounce loop reaches first)
        if args.config == "c2":
            sec, over, key = workloads.get("c2_refcaps"), None, "secondary_refcaps_Msamples_s"
        else:
            sec, over, key = wl, {"MAX_DIFF_BOUNCES": 12}, "secondary_truedepth_Msamples_s"
        workloads.configure(job.r, sec, over)
        job.step(0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(args.steps):
            job.step(i)
        torch.cuda.synchronize()
        out[key] = round(W * H * sec["spp"] * args.steps / (time.perf_counter() - t1) / 1e6, 3)
    if not args.no_cpu_baseline and world == 1:  # rank 0 at N=1 only
        # the JS integrator covers every BASELINE workload's features
        # (quadrics, SDFs, media, MIS, ReSTIR, spectral, triangle models)
        js = cpu_baseline_js(wl)
        c_port = cpu_baseline_c(wl)
        out["cpu_baseline"] = js if js and "value" in js else c_port
        out["cpu_baseline_c"] = c_port  # the C oracle on the same workload (OpenMP)
        if js and "error" in js:
            out["cpu_baseline_js_error"] = js["error"][-160:]
    print(json.dumps(out), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

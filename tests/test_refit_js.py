"""The addon's updateModel (rt0_update_model from the reference's host
language): setModel, render, updateModel, render in a node script; the images
differ, and the second is the Python host's, bit for bit as in test_js.py.
"""
import json
import os
import shutil

import numpy as np
import pytest

import rt0
from rt0 import meshes as M

from test_js import VIEWPORT, run_node

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(REPO, "raytracer-0_amd", "js",
                                                                                "rt0.node")),
                                reason="node or the rt0.node addon is missing")


def test_addon_exports_update_model():
    assert run_node("const v = require(%r); console.log(typeof v.addon.updateModel);" % VIEWPORT).strip() == "function"


@pytest.mark.gpu
def test_js_update_model_matches_python(cfgs, gpu_required, tmp_path):
    cfg = [c for c in cfgs["configs"] if c["name"] == "tri_models"][0]
    scene, sdf = rt0.scene_strings(cfg, cfgs)
    defines, consts = rt0.config_strings(cfg)
    cam = cfg.get("camera") or cfgs["default_camera"]
    models = [M.icosphere(2), M.wavy_icosphere(2)]
    new = M.wavy_icosphere(2, amp=0.15, freq=4.0)[0]
    files = {}
    for name, a in (("v0", models[0][0]), ("t0", models[0][1]), ("v1", models[1][0]), ("t1", models[1][1]),
                    ("new", new)):
        files[name] = str(tmp_path / (name + ".bin"))
        np.ascontiguousarray(a).tofile(files[name])
    src = """
const fs = require('fs');
const v = require(%r);
const a = v.addon, f = %s;
const f32 = p => { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4); };
const i32 = p => { const b = fs.readFileSync(p); return new Int32Array(b.buffer, b.byteOffset, b.length / 4); };
const h = a.create(48, 48, 0);
a.setConfig(h, %s, %s);
a.setScene(h, %s, %s);
a.setCamera(h, %s, %s, %s);
a.setModel(h, 0, f32(f.v0), i32(f.t0));
a.setModel(h, 1, f32(f.v1), i32(f.t1));
a.render(h, 1, 1, 0);
fs.writeFileSync(%r, Buffer.from(a.readAccum(h).buffer));
a.updateModel(h, 1, f32(f.new));
a.clear(h);
a.render(h, 1, 1, 0);
fs.writeFileSync(%r, Buffer.from(a.readAccum(h).buffer));
let threw = '';
try { a.updateModel(h, 1, new Float32Array(9)); } catch (e) { threw = e.message; }
console.log(JSON.stringify(threw));
""" % (VIEWPORT, json.dumps(files), json.dumps(defines), json.dumps(consts), json.dumps(scene), json.dumps(sdf),
       json.dumps(cam["origin"]), json.dumps(cam["lookat"]),
       json.dumps([cam["fov"], cam["aperture"], cam["focalLength"]]), str(tmp_path / "a.bin"), str(tmp_path / "b.bin"))
    threw = json.loads(run_node(src).strip().splitlines()[-1])
    assert "-1" in threw, threw  # RT0_E_ARG for a wrong vertex count
    a = np.fromfile(str(tmp_path / "a.bin"), np.float32).reshape(48, 48, 4)
    b = np.fromfile(str(tmp_path / "b.bin"), np.float32).reshape(48, 48, 4)
    assert not np.array_equal(a, b)
    r = rt0.Renderer(48, 48)
    rt0.configure(r, cfg, cfgs)
    for k, (v, t) in enumerate(models):
        r.set_model(k, v, t)
    r.render(1, 1)
    assert np.array_equal(r.read_accum(), a)
    r.update_model(1, new)
    r.clear()
    r.render(1, 1)
    got = r.read_accum()
    assert np.array_equal(got, b), (got != b).any(-1).mean()

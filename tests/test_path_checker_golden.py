"""CPU test: the three ground-truth checkers (or_render_path and or_render_path_unbiased of tests/cpp/path_oracle.c,
or_render_direct_mis of oracle/restir_oracle.c) against frames recorded from them before their shared parts -- the
mis_surf builder and the pixel driver -- were written once (tests/golden/path_checker_frames.json: the SHA-256 of the
C-contiguous float32 (H, W, 3) frame and the ray count).  The kernels are held to these checkers bit for bit, so the
checkers have a pin of their own.  Frame index 1, no sky: the sky lookup is the host's atan2f, everything else goes
through rs_libm.h, and the hashes do not depend on the oracle's thread count."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import path_oracle as PO
from restir_amd import params as P
from restir_amd import scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_checker_frames.json")
FRAME = 1
# scene, params, W, H, spp, max_bounces, render_path keywords
CASES = {
    "c1": ("cornell", P.default_params, 32, 24, 2, 5, {}),
    "rr": ("cornell", P.default_params, 25, 19, 3, 8, {}),                  # roulette live past bounce 5
    "phong": ("sponza", P.c3_params, 32, 18, 2, 5, {}),
    "gi0": ("cornell", P.default_params, 32, 24, 2, 5, dict(calc_gi=False)),
    "di0": ("cornell", P.default_params, 32, 24, 2, 5, dict(calc_di=False)),
}
SCENES = {"cornell": lambda: scenes.cornell_box(8), "sponza": lambda: scenes.sponza_like(30_000, 128)}
_scenes = {}


def _scene(key):
    if key not in _scenes:
        sc = SCENES[key]()
        _scenes[key] = (sc, O.OracleScene(sc))
    return _scenes[key]


def _entry(frame, rays):
    return {"sha256": hashlib.sha256(np.ascontiguousarray(frame, np.float32).tobytes()).hexdigest(), "rays": rays}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("which", list(CASES))
def test_checker_frames_are_the_recorded_ones(golden, which):
    key, prm_fn, W, H, spp, mb, kw = CASES[which]
    (sc, os_), prm, o = _scene(key), prm_fn(), O.OracleRenderer(W, H)
    got = {}
    with O.num_threads(4):
        got["reference"] = _entry(PO.render_path(o, os_, sc.camera, prm, FRAME, spp, max_bounces=mb, **kw), o.rays)
        got["unbiased"] = _entry(PO.render_path(o, os_, sc.camera, prm, FRAME, spp, max_bounces=mb, unbiased=True, **kw),
                                 o.rays)
        if not kw:                                                           # the direct integrator has no switches
            got["direct_mis"] = _entry(o.render_direct_mis(os_, sc.camera, prm, FRAME, spp), o.rays)
    assert got == golden[which]


def test_gi_off_is_the_direct_mis_frame(golden):
    """`gi0` is `c1` with calc_gi off: the reference's estimator renders the direct-MIS frame, ray count included"""
    key, prm_fn, W, H, spp, mb, kw = CASES["gi0"]
    (sc, os_), prm, o = _scene(key), prm_fn(), O.OracleRenderer(W, H)
    with O.num_threads(4):
        path = _entry(PO.render_path(o, os_, sc.camera, prm, FRAME, spp, max_bounces=mb, **kw), o.rays)
        direct = _entry(o.render_direct_mis(os_, sc.camera, prm, FRAME, spp), o.rays)
    assert path == direct == golden["gi0"]["reference"] == golden["c1"]["direct_mis"]

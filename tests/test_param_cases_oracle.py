"""CPU tests: what tests/test_gpu_param_sweep.py relies on, asserted on the oracle alone -- every case of
tests/param_cases.py changes the frame it is compared on (a case that changes nothing tests nothing), every frame is
finite, the confidence caps give the maxima the table names, the radii give the halos it names, and the two ranges
the library enforces are the header's."""
import os
import re

import numpy as np
import pytest

import material_cases as M
import param_cases as C
from restir_amd import params as P
from restir_amd.distributed import halo_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARDED = [c for c in C.ALL if c not in C.AGREE]


@pytest.mark.parametrize("case", GUARDED)
def test_case_changes_the_frame(case):
    """The effect guard -- a condition on the inputs, not a tolerance: the oracle's last frame differs from the base
    run's, at the same size, in at least MIN_CHANGED of the pixels."""
    base, run = C.oracle(None, C.size(case)), C.oracle(case)
    share = [C.changed_share(a, b) for a, b in zip(run.frames, base.frames)]
    print(f"[params] {case}: changed share per frame {' '.join(f'{s:.3f}' for s in share)}, fields {C.changed_fields(case)}")
    assert all(np.isfinite(f).all() for f in run.frames)
    assert share[-1] >= C.MIN_CHANGED, f"{case} changes {share[-1]:.3f} of the last frame"
    if case == "bg_color":                         # the miss pixels alone
        assert M.same(run.reservoirs, base.reservoirs)
    else:
        assert not M.same(run.reservoirs, base.reservoirs)


@pytest.mark.parametrize("case", list(C.AGREE))
def test_case_agrees(case):
    """Different parameters, the same run: frames, G-buffer and reservoirs"""
    other = C.AGREE[case][1]
    assert C.changed_fields(case) and C.fields(case) != C.fields(other)
    run = C.oracle(case)
    assert all(np.isfinite(f).all() for f in run.frames)
    M.assert_same_render(run, C.oracle(other, C.size(case)), f"{case} vs {other or 'base'}")
    if case == "small_1x1":                        # why it agrees: the pixel is a miss, its reservoir empty
        assert run.gbuffer[0, 0, 16] == 0 and run.reservoirs[0, 0, 11] == 0


def test_one_field_per_case():
    for case in C.CASES:
        if case != "combined":
            assert len(C.changed_fields(case)) == 1, case
    assert len(C.changed_fields("combined")) == len(C.COMBINED) == 7
    moved = {f for case in C.ALL for f in C.changed_fields(case)}
    # every field but the switches BASE turns on, the MIS mode, use_skybox and debug_reprojection, which other files move
    assert moved == {"m_area", "m_brdf", "spatial_neighbors", "spatial_passes", "confidence_cap", "spatial_radius",
                     "min_normal_similarity", "max_depth_difference", "bg_color", "tnear_offset", "tfar_offset",
                     "normal_offset", "seed"}


def test_form_tables_name_cases():
    for table in (C.OFFSETS, C.SORTED, C.SPLIT_AHEAD, C.TILES, C.MGPU, C.CONF_MAX, C.HALO):
        assert set(table) <= set(C.CASES)
    assert P.CONSTANT == C.params().spatial_mis and C.params().spatial_neighbors + 1 <= 9    # the sorted spatial pass takes BASE


@pytest.mark.parametrize("case", list(C.CONF_MAX))
def test_confidence_maxima(case):
    conf = C.oracle(case).reservoirs[..., 11]
    assert conf.min() >= 0 and conf.max() == C.CONF_MAX[case]
    assert (conf == np.floor(conf)).all()


def test_largest_cap_cannot_overflow():
    """65 capped confidences -- the pixel's and 64 neighbours' -- sum in an int32, and one more cap does not"""
    assert 65 * P.MAX_CONFIDENCE_CAP <= 2**31 - 1 < 65 * (P.MAX_CONFIDENCE_CAP + 1)
    assert C.params("cap_max").confidence_cap == P.MAX_CONFIDENCE_CAP
    assert C.params("nbr_64").spatial_neighbors == 64


def test_halo_table():
    for case, rows in C.HALO.items():
        assert halo_rows(C.params(case)) == rows, case
    assert halo_rows(C.params("passes_0", spatial_radius=400.0)) == 0
    assert halo_rows(C.params("radius_1e6")) == 1000
    assert halo_rows(C.params(spatial_radius=P.MAX_SPATIAL_RADIUS)) == 2**28
    w, h = C.TILE_SIZE
    assert h // 3 >= max(C.HALO.values()) > h // 4          # 2 and 3 ranks hold a 20-row halo, 4 ranks do not


@pytest.mark.parametrize("kind", C.GT_KINDS)
def test_ground_truth_fields_change_the_frame(kind):
    """The effect guard of the ground truths: the offsets, the seed and the background moved together"""
    moved, default = C.oracle_truths(True)[kind], C.oracle_truths(False)[kind]
    for f in range(C.GT_FRAMES):
        share = C.changed_share(moved[f], default[f])
        print(f"[params] {kind} frame {f}: changed share {share:.3f}")
        assert np.isfinite(moved[f]).all() and share >= C.MIN_CHANGED
    # the background alone reaches the frame: a miss pixel shows it
    assert (moved[0] == np.asarray(C.BG, np.float32)).all(-1).any()


def test_ranges_are_the_headers():
    text = open(os.path.join(ROOT, "include", "restir_c.h")).read()
    cap = re.search(r"#define RS_MAX_CONFIDENCE_CAP (\d+)\s", text)
    rad = re.search(r"#define RS_MAX_SPATIAL_RADIUS ([0-9.]+)f\s", text)
    assert int(cap.group(1)) == P.MAX_CONFIDENCE_CAP
    assert float(rad.group(1)) == P.MAX_SPATIAL_RADIUS == float(np.float32(P.MAX_SPATIAL_RADIUS)) == 2.0**56

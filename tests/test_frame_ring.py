"""CPU test of the frame-in-flight ring bookkeeping (restir-embree_amd/csrc/rs_frame_ring.h -- the code
rs_tile_begin calls to pick a frame's lane, its reservoir buffers and its G-buffer slot, and to size its launches):
tests/cpp/frame_ring_harness.cpp exposes it; every pick is checked for the invariants run-ahead relies on and against
the restatement below, which is written from the header's comment block, not from its code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "frame_ring_harness.cpp")
HDR = os.path.join(ROOT, "restir-embree_amd", "csrc", "rs_frame_ring.h")
SO = os.path.join(ROOT, "tests", "cpp", "_build", "libframe_ring_harness.so")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    lib = ctypes.CDLL(SO)
    lib.fr_new.restype = ctypes.c_void_p
    lib.fr_free.argtypes = [ctypes.c_void_p]
    lib.fr_begin.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.fr_finish.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.fr_grid.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_uint)]
    lib.fr_grid_waves.restype = ctypes.c_ulonglong
    lib.fr_grid_waves.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_int]
    lib.fr_count_slot_need.restype = ctypes.c_ulonglong
    lib.fr_count_slot_need.argtypes = [ctypes.c_int] * 7 + [ctypes.c_ulonglong]
    return lib


class PyRing:
    """The rules as the comment block of rs_frame_ring.h states them."""

    def __init__(self, max_ahead):
        self.n_r, self.n_g = 3 * max_ahead + 2, max_ahead + 2
        self.final = 2              # the buffer a fresh context calls the last frame's
        self.touched = []           # per earlier frame, most recent first: the buffers it wrote or read
        self.g = 0
        self.seq = 0

    def begin(self, D, fb_ring):
        lane = self.seq % (D + 1) if D > 0 else (self.seq & 1 if fb_ring == 2 else 0)
        self.seq += 1
        last = self.final
        busy = {last}.union(*self.touched[:D]) if D else {last}
        free = [i for i in range(self.n_r) if i not in busy]
        ra, rb = free[0], free[1]                   # the two lowest-numbered free buffers
        self.touched.insert(0, {ra, rb, last})
        gprev, self.g = self.g, (self.g + 1) % self.n_g
        return lane, ra, rb, last, self.g, gprev


@pytest.mark.parametrize("D0", [0, 1, 2])
def test_ring_picks_keep_frames_in_flight_apart(L, D0):
    A = L.fr_max_ahead()
    assert D0 <= A and L.fr_rring() == 3 * A + 2 and L.fr_gring() == A + 2
    rng = np.random.default_rng(D0)
    st, py = L.fr_new(), PyRing(A)
    out = (ctypes.c_int * 6)()
    D, hist, final = D0, [], 2
    try:
        for f in range(3000):
            if rng.integers(61) == 0:               # a depth change at an arbitrary frame (every depth 0..A)
                D = int(rng.integers(A + 1))
            fb_ring = int(rng.integers(1, 3))
            L.fr_begin(st, D, fb_ring, out)
            lane, ra, rb, last, gnew, gprev = list(out)
            assert ra != rb and 0 <= ra < L.fr_rring() and 0 <= rb < L.fr_rring(), (f, D, ra, rb)
            assert last == final and last not in (ra, rb), (f, D, ra, rb, last)
            for g, t in enumerate(hist[:D]):        # the D frames before it may still run
                assert ra not in t and rb not in t, (f, D, g, ra, rb, t)
            assert lane == ((f % (D + 1)) if D > 0 else ((f & 1) if fb_ring == 2 else 0)), (f, D, lane)
            assert gprev == (gnew - 1) % L.fr_gring() and 0 <= gnew < L.fr_gring()
            assert (lane, ra, rb, last, gnew, gprev) == py.begin(D, fb_ring), (f, D)
            hist.insert(0, (ra, rb, last))
            final = (ra, rb)[int(rng.integers(2))]  # temporal / spatial passes end in either buffer
            L.fr_finish(st, final)
            py.final = final
    finally:
        L.fr_free(st)


def test_grids_and_count_slot_need(L):
    g = (ctypes.c_uint * 4)()
    cdiv = lambda a, b: -(-a // b)
    for W, ya, yb in [(1920, 0, 1080), (96, 0, 64), (97, 5, 6), (1, 0, 1), (3840, 130, 275), (64, 16, 48)]:
        L.fr_grid(W, ya, yb, g)
        assert list(g) == [cdiv(W, 16), cdiv(yb - ya, 16), cdiv(W, 8), cdiv(yb - ya, 8)]
        assert L.fr_grid_waves(g[0], g[1], 4) == 4 * g[0] * g[1]
        for margin, split, passes, extra in [(0, 0, 0, 0), (5, 0, 2, 7), (9, 3, 1, 0), (0, 2, -1, 11)]:
            gy0, gy1 = max(0, ya - margin), yb + margin
            band = 4 * cdiv(W, 16) * cdiv(yb - ya, 16)
            init = split * cdiv(W, 8) * cdiv(gy1 - gy0, 8) if split else 4 * cdiv(W, 16) * cdiv(gy1 - gy0, 16)
            # the initial launch + four band launches' worth (visibility, temporal, shade, one spare) + the spatial passes
            assert L.fr_count_slot_need(W, gy0, gy1, ya, yb, split, passes, extra) == init + 4 * band + max(0, passes) * band + extra

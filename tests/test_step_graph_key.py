"""step_graph.pick_key: which cached captured step a step may replay -- same step shape, and every capacity c of the cached step
within m <= c <= 3 m + 16384 of the need m = int(rays * samples per ray * 1.08) + 1024.  Pure: no device, no library."""
import os
import subprocess
import sys

from robust_e_nerf_amd import step_graph

SHAPE = (2048, 1.0, "begun", True, True, (("position", (2048, 2), "torch.int64"),), False, False, 1e-3)
RAYS, SPR = [4096, 2048], (40.0, 9.5)
NEED = tuple(tuple(int(n * s * 1.08) + 1024 for s in SPR) for n in RAYS)
FRESH = ((1 << 20, 1 << 18), (1 << 19, 1 << 17))          # what SampleCounts.capacities would give now


def _pick(caps, shape=SHAPE):
    key = (caps,) + shape
    return key, step_graph.pick_key({key: None}, FRESH, SHAPE, RAYS, SPR)


def test_every_capacity_between_the_need_and_three_times_it_plus_16384_fits():
    for r in range(2):
        for j in range(2):
            m = NEED[r][j]
            for c, fits in ((m, True), (m - 1, False), (3 * m + 16384, True), (3 * m + 16385, False)):
                caps = tuple(tuple(c if (rr, jj) == (r, j) else NEED[rr][jj] for jj in range(2)) for rr in range(2))
                key, got = _pick(caps)
                assert got == (key if fits else (FRESH,) + SHAPE), (r, j, c, fits)


def test_another_step_shape_misses():
    key, got = _pick(NEED, shape=(1024,) + SHAPE[1:])
    assert got == (FRESH,) + SHAPE
    key, got = _pick(NEED, shape=SHAPE[:-1] + (0.0,))
    assert got == (FRESH,) + SHAPE
    key, got = _pick(NEED)
    assert got is key


def test_the_first_fitting_key_wins_and_an_empty_cache_gives_the_fresh_key():
    a, b = (NEED,) + SHAPE, (tuple((3 * x, 3 * y) for x, y in NEED),) + SHAPE
    assert step_graph.pick_key({a: None, b: None}, FRESH, SHAPE, RAYS, SPR) is a
    assert step_graph.pick_key({b: None, a: None}, FRESH, SHAPE, RAYS, SPR) is b
    assert step_graph.pick_key({}, list(FRESH), SHAPE, RAYS, SPR) == (FRESH,) + SHAPE


def test_importing_and_calling_it_loads_no_library():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from robust_e_nerf_amd import _lib, step_graph\n"
            "k = step_graph.pick_key({}, [(1, 2)], ('s',), [10], (1.0, 1.0))\n"
            "assert k == (((1, 2),), 's') and _lib._lib is None, (k, _lib._lib)\n")
    subprocess.run([sys.executable, "-c", code], cwd=repo, check=True)

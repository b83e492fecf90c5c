"""sample_counts.SampleCounts / CountLog on the host: how capacities are sized and learnt, what an overflow may and may not touch,
and that a repeat always ends.  No GPU, no library: stand-ins for the Trainer, and logs that are objects with a wait()."""
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import pytest
import torch

from robust_e_nerf_amd.sample_counts import CountLog, SampleCounts


def _learnt():
    sc = SampleCounts()
    sc.learn(4096, 4096 * 40, 4096 * 19 // 2)
    assert sc.spr == (40.0, 9.5)
    return sc


def test_no_capacities_before_anything_was_learnt():
    assert SampleCounts().capacities(4096) is None


@pytest.mark.parametrize("n", [1, 777, 4096, 131072])
def test_capacities_are_the_need_rounded_up_to_an_eighth_octave(n):
    caps = _learnt().capacities(n)
    assert len(caps) == 2
    for c, s in zip(caps, (40.0, 9.5)):
        x = int(n * s * 1.25) + 4096
        q = max(1024, 1 << max(0, x.bit_length() - 4))
        assert c >= x and c % q == 0 and c - x < q
        assert c == (x + q - 1) // q * q


def test_a_capacity_of_2_to_the_23_or_more_gives_none():
    sc = _learnt()
    assert int(262144 * 40.0 * 1.25) + 4096 >= 1 << 23
    assert sc.capacities(262144) is None


def test_learning_goes_up_at_once_and_down_slowly():
    sc = SampleCounts()
    sc.learn(1000, 30000, 7000)
    assert sc.spr == (30000 / 1000, 7000 / 1000)                 # the first: exactly the counts per ray
    sc.learn(500, 20000, 4000)                                   # (40, 8): both larger
    assert sc.spr == (20000 / 500, 4000 / 500)
    old = sc.spr
    sc.learn(1000, 20000, 9000)                                  # (20, 9): one smaller, one larger
    a = 20000 / 1000
    assert sc.spr == (max(a, 0.75 * old[0] + 0.25 * a), 9000 / 1000)
    assert a < sc.spr[0] < old[0]
    sc.learn(0, 0, 0)                                            # an empty render divides by nothing
    assert sc.spr == tuple(0.75 * b for b in (max(a, 0.75 * old[0] + 0.25 * a), 9.0))


class _Log:
    def __init__(self, n_rays, values):
        self.n_rays, self._values = n_rays, values

    def wait(self):
        return self._values


class _Recording(SampleCounts):
    def __init__(self):
        super().__init__()
        self.learnt = []

    def learn(self, n_rays, marched, kept):
        self.learnt.append((n_rays, marched, kept))
        super().learn(n_rays, marched, kept)


@pytest.mark.parametrize("values", [[(900, 1, 0, 0)], [(900, 0, 300, 1)], [(900, 0, 300, 0), (500, 0, 100, 2)]])
def test_an_overflow_teaches_nothing_and_writes_nothing(values):
    sc = _Recording()
    sc.learn(100, 4000, 1000)
    spr, sc.learnt = sc.spr, []
    passes = [(_Log(100, v), dict(n=-1, n_marched=-2)) for v in values]
    assert sc.settle(passes) is True
    assert sc.spr == spr and sc.learnt == []
    assert all(aux == dict(n=-1, n_marched=-2) for _, aux in passes)


def test_counts_that_fitted_reach_the_auxes_and_the_capacities_in_order():
    sc = _Recording()
    passes = [(_Log(200, (9000, 0, 3000, 0)), dict(n=-1, n_marched=-2, rays=200)), (_Log(100, (5000, 0, 1000, 0)), dict(n=-1))]
    assert sc.settle(passes) is False
    assert passes[0][1] == dict(n=3000, n_marched=9000, rays=200)
    assert passes[1][1] == dict(n=1000)                          # no "n_marched" where there was none
    assert sc.learnt == [(200, 9000, 3000), (100, 5000, 1000)]
    want = SampleCounts()
    want.learn(200, 9000, 3000)
    want.learn(100, 5000, 1000)
    assert sc.spr == want.spr


def _trainer(calls):
    return NS(fronts=NS(reset=lambda: calls.append("reset")))


def test_a_repeat_runs_with_the_flag_up_after_the_fronts_were_reset():
    sc, calls = SampleCounts(), []

    def fn():
        calls.append(("fn", sc.host_repeat))
        return "out"

    assert sc.host_repeat is False and sc.overflows == 0
    assert sc.repeat(_trainer(calls), fn) == "out"
    assert calls == ["reset", ("fn", True)]
    assert sc.host_repeat is False and sc.overflows == 1


def test_a_repeat_that_raises_still_clears_the_flag():
    sc, calls = SampleCounts(), []

    def fn():
        calls.append(("fn", sc.host_repeat))
        raise KeyError("from the pass")

    with pytest.raises(KeyError, match="from the pass"):
        sc.repeat(_trainer(calls), fn)
    assert calls == ["reset", ("fn", True)]
    assert sc.host_repeat is False and sc.overflows == 1


def test_mode():
    sc = SampleCounts()
    assert sc.mode(False) is False and sc.mode(True) is True
    sc.host_repeat = True
    assert sc.mode(True) == "learn" and sc.mode(False) is False


def test_a_polled_count_log_over_cpu_tensors():
    stats, words = torch.tensor([900, 0, 300, 0]), torch.full((4,), -7)
    log = CountLog(64, (1024, 1024), stats, words, polled=True)
    assert log.ev is None and log.values is None
    assert log.wait() == (900, 0, 300, 0) and all(type(v) is int for v in log.values)
    words.fill_(5)
    assert log.wait() == (900, 0, 300, 0)                        # cached: the words are not read again
    assert log.overflowed is False
    log.arm()
    assert words.tolist() == [-1] * 4 and log.values is None
    for landed, over in (([900, 1, 0, 0], True), ([900, 0, 300, 2], True), ([900, 0, 0, 0], False)):
        log.arm()
        words.copy_(torch.tensor(landed))                        # (what a replay's copy node does)
        assert log.overflowed is over and log.values == tuple(landed)


def test_importing_it_loads_no_library():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from robust_e_nerf_amd import _lib, sample_counts\n"
            "assert sample_counts.SampleCounts().capacities(8) is None and _lib._lib is None, _lib._lib\n")
    subprocess.run([sys.executable, "-c", code], cwd=repo, check=True)

"""The pose and ray kernels, every copy on its own, against the float64 reference of tests/pose_reference.py on the same
float32 tables: `ops.trajectory` / `ops.raygen` / `ops.pose_rays` (csrc/ren_pose.hip), `jvp.trajectory_jvp` / `raygen_jvp`
(csrc/ren_jvp.hip), `jvp.trajectory_jvp2` / `raygen_jvp2` (csrc/ren_jvp2.hip).  The three files each carry their own binary
search, clamps, shortest-path flip, Taylor / trigonometric branches and quaternion-to-matrix expansion; nothing else holds
them to one another.  Tables: quaternion sign flips, relative angles from 0 over both sides of the 1e-3 branches to 3.1 rad,
bins of one tick (1024 ns) to 4e7 ns at timestamps of 1.7e18 ns, queries at w = 0, on every knot and around torch.lerp's
switch at 0.5; two knots; 1025 knots; the orbit golden's table queried on its knots; timestamps outside the table.

Error measure: absolute error of p, R, o, d; time derivatives per unit of the interpolation weight (first ones times bin,
second ones times bin^2), which puts a 1024 ns bin and a 4e7 ns bin on one scale."""
import numpy as np
import pytest
import torch

import pose_reference as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# YARDSTICK: max |float32 evaluation - float64 evaluation| of tests/pose_reference.py (numpy, on the CPU) on the case's own inputs,
# per quantity -- what the float32 chain itself costs; it owes nothing to the kernels (pose_reference.yardsticks() measures it,
# tests/test_pose_reference_cpu.py holds these figures to it).  "raygen": the ray generators alone on the adversarial case's
# float64 pose rounded to float32; "pose_rays": pose + ray in one, the worst of the four layouts below.
# BOUND = 4 x YARDSTICK is what a kernel may deviate from the float64 reference: the device's atan2f / sinf / cosf are good to
# a couple of ulp where the host's are nearly correctly rounded, and the compiler contracts the chain's multiply-adds its own way.
# A yardstick of 0 is an exact quantity (a copied position, lerp at w = 1): the kernel has to be exact there too.
# Every bound on a value is far below the 1e-5 of the largest entry the golden tests of tests/test_gpu_parity.py use.
YARDSTICK = {
    "adversarial": {"p": 4.54e-07, "R": 3.25e-07, "dp": 4.92e-07, "dR": 7.84e-07, "ddR": 3.22e-06},
    "outside": {"p": 8.05e-07, "R": 3.53e-07, "dp": 1.7e-07, "dR": 7.44e-07, "ddR": 2.16e-06},
    "two_knots": {"p": 8.3e-08, "R": 3.37e-07, "dp": 5.26e-08, "dR": 8.76e-07, "ddR": 2.58e-06},
    "random_1025": {"p": 5.72e-07, "R": 3.53e-07, "dp": 7.83e-07, "dR": 1.07e-06, "ddR": 3.57e-06},
    "orbit_knots": {"p": 0.0, "R": 2.22e-07, "dp": 1.87e-09, "dR": 7.31e-08, "ddR": 1.09e-09},
    "raygen": {"o": 0.0, "d": 9.6e-08, "do": 0.0, "dd": 3.43e-07, "ddd": 1.71e-06},
    "pose_rays": {"o": 4.54e-07, "d": 2.6e-07},
}
BOUND = {case: {q: 4 * v for q, v in qs.items()} for case, qs in YARDSTICK.items()}

COPIES = ("fwd", "jvp", "jvp2")
BATCHES = (1, 255, 256, 257)                      # the launches use 256-thread blocks


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, jvp, ops
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, jvp


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                   # a copy: the shared cases are read-only


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def trajectory(amd, copy, ts, table):
    """one of the three trajectory kernels -> its outputs on the host, in the order p, R, dp/dt, dR/dt, d2R/dt2"""
    ops, jvp = amd
    fn = {"fwd": ops.trajectory, "jvp": jvp.trajectory_jvp, "jvp2": jvp.trajectory_jvp2}[copy]
    p, R, *rest = host(fn(dev(ts), *(dev(a) for a in table)))
    assert len(rest) == {"fwd": 0, "jvp": 2, "jvp2": 3}[copy] and p.dtype == R.dtype == np.float32
    assert p.shape == (len(ts), 3) and R.shape == (len(ts), 3, 3)
    return (p, R, *rest)


def raygen(amd, copy, Kinv, px, pose):
    """one of the three ray generators on the pose (and the derivatives it takes) -> o, d, do/dt, dd/dt, d2d/dt2"""
    ops, jvp = amd
    fn, n_in = {"fwd": (ops.raygen, 2), "jvp": (jvp.raygen_jvp, 4), "jvp2": (jvp.raygen_jvp2, 5)}[copy]
    out = host(fn(dev(Kinv), dev(px), *(dev(a) for a in pose[:n_in])))
    assert len(out) == n_in and all(a.shape == (len(px), 3) and a.dtype == np.float32 for a in out)
    return out


def hold(tag, errs, bound):
    print(tag, {k: f"{v:.3g} (bound {bound[k]:.3g})" for k, v in errs.items()})
    for k, v in errs.items():
        assert np.isfinite(v) and v <= bound[k], (tag, k, v, bound[k])


# ---------------------------------------------------------------------------------------------------- trajectory
@pytest.mark.parametrize("copy", COPIES)
@pytest.mark.parametrize("name", ["adversarial", "two_knots", "random_1025", "orbit_knots"])
def test_trajectory_vs_float64_reference(amd, name, copy):
    """every copy against the reference, case by case: flips, both sides of every branch, knots, one-tick bins, C = 2,
    11 levels of search, the orbit table on its knots"""
    c = pr.case(name)
    if name in ("adversarial", "random_1025"):
        assert pr.min_abs_dot(c["table"][2]) >= pr.MIN_ABS_DOT          # the flip cannot be decided differently in float32
    if name == "two_knots":
        assert len(c["table"][0]) == 2
    got = trajectory(amd, copy, c["ts"], c["table"])
    hold(f"{name}/{copy}", pr.pose_errors(got, c["pose"], c["bin"]), BOUND[name])


@pytest.mark.parametrize("copy", COPIES)
def test_trajectory_outside_the_table(amd, copy):
    """before the first knot the first pose is held with zero derivatives, after the last knot the last segment is extrapolated
    (the reference project asserts such timestamps away)"""
    c = pr.case("outside")
    got = trajectory(amd, copy, c["ts"], c["table"])
    hold(f"outside/{copy}", pr.pose_errors(got, c["pose"], c["bin"]), BOUND["outside"])
    before = c["ts"] < float(c["table"][0][0])
    assert before.sum() == 5 and (c["ts"][~before] > float(c["table"][0][-1])).all()
    assert (got[0][before] == c["table"][1][0]).all()                  # held exactly: lerp(a, a, w) = a
    if copy != "fwd":
        assert (got[2][before] == 0).all()                             # (a - a) / bin


@pytest.mark.parametrize("copy", COPIES)
def test_trajectory_batch_sizes(amd, copy):
    """one thread, one short of a block, a block, one more than a block"""
    c = pr.case("adversarial")
    for B in BATCHES:
        idx = np.arange(B) % len(c["ts"]) if B > 1 else np.array([40])
        got = trajectory(amd, copy, c["ts"][idx], c["table"])
        want = tuple(a[idx] for a in c["pose"])
        hold(f"B={B}/{copy}", pr.pose_errors(got, want, c["bin"][idx]), BOUND["adversarial"])


# ---------------------------------------------------------------------------------------------------- ray generators
@pytest.mark.parametrize("copy", COPIES)
def test_raygen_vs_float64_reference(amd, copy):
    """each ray generator alone: the float64 rays of the SAME float32 pose and derivatives; principal point, image corners, a
    Kinv with skew"""
    pose32, bin_, px = pr.ray_inputs()
    want = pr.rays(pr.KINV_SKEW, px, *pose32)
    for B in (len(px),) + BATCHES:
        idx = np.arange(B) % len(px) if B > 1 else np.array([40])
        got = raygen(amd, copy, pr.KINV_SKEW, px[idx], tuple(a[idx] for a in pose32))
        hold(f"raygen B={B}/{copy}", pr.ray_errors(got, tuple(a[idx] for a in want), bin_[idx]), BOUND["raygen"])
        assert (got[0] == pose32[0][idx]).all()                        # o is the position, copied
        if copy != "fwd":
            assert (got[2] == pose32[2][idx]).all()


# ---------------------------------------------------------------------------------------------------- pose + ray in one launch
@pytest.mark.parametrize("R,px_rows", pr.POSE_RAYS_LAYOUTS, ids=[f"R{a}-px{b}" for a, b in pr.POSE_RAYS_LAYOUTS])
def test_pose_rays_vs_float64_reference(amd, R, px_rows):
    """the launch a training step uses: ray i goes through pixel i % px_rows -- one pixel per ray, the step's start / end
    layout R = 2 px_rows, a single pixel, and a row count that does not divide R"""
    ops, _ = amd
    c = pr.case("adversarial")
    ts, px, want = pr.pose_rays_case(R, px_rows)
    o, d = host(ops.pose_rays(dev(ts), dev(px), dev(pr.KINV_SKEW), *(dev(a) for a in c["table"])))
    assert o.shape == d.shape == (R, 3)
    hold(f"pose_rays R={R} px_rows={px_rows}", pr.ray_errors((o, d), want, np.ones(R)), BOUND["pose_rays"])


# ---------------------------------------------------------------------------------------------------- empty batches
def test_empty_batches_return_without_a_launch(amd):
    ops, jvp = amd
    c = pr.case("adversarial")
    table = tuple(dev(a) for a in c["table"])
    Kinv = dev(pr.KINV_SKEW)
    ts0 = torch.empty(0, dtype=torch.float64, device=DEV)
    e3, e33, px0 = torch.empty(0, 3, device=DEV), torch.empty(0, 3, 3, device=DEV), torch.empty(0, 2, device=DEV)
    outs = [ops.trajectory(ts0, *table), jvp.trajectory_jvp(ts0, *table), jvp.trajectory_jvp2(ts0, *table),
            ops.raygen(Kinv, px0, e3, e33), jvp.raygen_jvp(Kinv, px0, e3, e33, e3, e33),
            jvp.raygen_jvp2(Kinv, px0, e3, e33, e3, e33, e33), ops.pose_rays(ts0, dev(pr.pixels(4)), Kinv, *table)]
    torch.cuda.synchronize()
    for out in outs:
        assert all(t.shape[0] == 0 for t in out)
    # the C entry points themselves: a count of 0 with real pointers is REN_OK and leaves the outputs alone
    from robust_e_nerf_amd import _lib
    from robust_e_nerf_amd.ops import _ptr, _stream
    ts1, px1 = dev(c["ts"][:4]), dev(pr.pixels(4))
    o, d = torch.full((4, 3), 7.0, device=DEV), torch.full((4, 3), 7.0, device=DEV)
    lib = _lib.load()
    assert lib.ren_trajectory_fwd(_ptr(ts1), 0, _ptr(table[0]), _ptr(table[1]), _ptr(table[2]), 16, _ptr(o), None, _stream()) == 0
    assert lib.ren_pose_rays_fwd(_ptr(ts1), 0, _ptr(px1), 4, _ptr(Kinv), _ptr(table[0]), _ptr(table[1]), _ptr(table[2]), 16,
                                 _ptr(o), _ptr(d), _stream()) == 0
    torch.cuda.synchronize()
    assert bool((o == 7).all()) and bool((d == 7).all())

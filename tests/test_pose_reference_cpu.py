"""tests/pose_reference.py against three things it was not written from: the torch oracle (oracle/trajectory.py) on float64
tables, torch autograd through that oracle, and central differences of its own first derivatives.  No GPU."""
import numpy as np
import pytest
import torch

import pose_reference as pr
from oracle import trajectory as otraj

EPS = float(np.finfo(np.float64).eps)


def t64(a):
    a = np.asarray(a)
    return torch.from_numpy(np.array(a, np.float64 if a.dtype.kind == "f" else a.dtype))


@pytest.fixture(scope="module")
def adv():
    """the adversarial table (timestamps of real size), its in-table queries, the float64 reference and the float64 oracle
    with a graph on the timestamps"""
    c = pr.case("adversarial")
    px = pr.pixels(len(c["ts"]))
    ts = t64(c["ts"]).requires_grad_()
    tab_ts, tab_pos, tab_quat = (t64(a) for a in c["table"])
    p, R = otraj.linear_trajectory(ts, tab_ts, tab_pos, tab_quat)
    o, d = otraj.pixel_params_to_ray(t64(pr.KINV_SKEW), t64(px), p, R)
    ref_rays = pr.rays(pr.KINV_SKEW, px, *c["pose"])
    return dict(c=c, px=px, ts=ts, p=p, R=R, o=o, d=d, rays=ref_rays)


def test_the_adversarial_table_is_what_it_says():
    tab_ts, tab_pos, tab_quat = pr.adversarial_table()
    assert tab_ts.dtype == np.int64 and len(tab_ts) == 16 and (tab_ts % 1024 == 0).all()
    assert (tab_ts.astype(np.float64).astype(np.int64) == tab_ts).all()             # every knot is exact as a double
    assert tab_ts[0] == pr.T0_REAL and abs(pr.T0_REAL - 1.7e18) < 1024
    widths = np.diff(tab_ts)
    assert widths.min() == 1024 == widths[pr.ONE_TICK_SEGMENT] and widths.max() <= 1024 * 40000
    assert pr.min_abs_dot(tab_quat) >= pr.MIN_ABS_DOT
    q = tab_quat.astype(np.float64)
    dots = (q[:-1] * q[1:]).sum(-1)
    assert (dots < 0).sum() >= 5 and (dots > 0).sum() >= 5                          # flips and no flips
    angles = 2 * np.arccos(np.clip(np.abs(dots), 0, 1))
    want = np.array(pr.ADVERSARIAL_ANGLES)
    big = want > 1e-2
    assert np.allclose(angles[big], want[big], rtol=1e-4)                           # below: float32 quaternions cannot say
    assert (np.abs(angles[~big] - want[~big]) < 1e-3).all()
    assert (q[1] == -q[0]).all() or (q[1] == q[0]).all()                            # the 0 rad segment repeats its quaternion
    # every query set: w = 0 once, a query on every interior knot and on the last one
    c = pr.case("adversarial")
    assert len(c["ts"]) == 1 + 15 * len(pr.QUERY_W)
    assert set(tab_ts.astype(np.float64)) <= set(c["ts"])
    assert pr.min_abs_dot(pr.case("random_1025")["table"][2]) >= pr.MIN_ABS_DOT


def test_pixels_cover_the_sensor():
    px = pr.pixels(136)
    hom = np.concatenate([px[:5].astype(np.float64), np.ones((5, 1))], -1) @ pr.KINV_SKEW.astype(np.float64).T
    assert np.abs(hom[0, :2]).max() < 1e-6                             # the principal point looks down the optical axis
    assert {tuple(r) for r in px[1:5].tolist()} == {(0.0, 0.0), (345.0, 0.0), (0.0, 259.0), (345.0, 259.0)}
    assert pr.KINV_SKEW[0, 1] != 0 and len(np.unique(px, axis=0)) > 100


def test_segment_rule_in_and_outside_the_table():
    tab = np.array([1000, 2000, 4000, 4100], np.int64)
    ts = np.array([1000, 1000.5, 2000, 2000.5, 4000, 4100, 4050, 999, -5e9, 4100.5, 9e9])
    left, right, bin_ = pr.segments(ts, tab)
    assert left.tolist() == [0, 0, 0, 1, 1, 2, 2, 0, 0, 2, 2]
    assert right.tolist() == [0, 1, 1, 2, 2, 3, 3, 0, 0, 3, 3]
    assert bin_.tolist() == [1000, 1000, 1000, 2000, 2000, 100, 100, 1000, 1000, 100, 100]
    pos = np.arange(12, dtype=np.float64).reshape(4, 3) ** 2
    quat = pr.random_table(4, seed=1)[2]
    p, R, dp, dR, ddR = pr.pose(ts, tab, pos, quat)
    for i in (7, 8):                                                                 # before the table: the first pose, held
        assert (p[i] == pos[0]).all() and (dp[i] == 0).all() and (dR[i] == 0).all() and (ddR[i] == 0).all()
        assert pr.max_abs(R[i], R[0]) < 4 * EPS
    # after the table: the last segment's straight line and constant angular velocity, continued
    assert np.allclose(p[9], pos[3] + (pos[3] - pos[2]) * 0.005, rtol=0, atol=1e-12) and (dp[9] == dp[5]).all()
    w = pr.pose_terms(ts, tab, pos, quat)["w64"]
    assert w[9] == 1.005 and w[10] > 1
    assert pr.max_abs(R[5].T @ R[9], R[6].T @ pr.pose(np.array([4050.5]), tab, pos, quat)[1][0]) < 16 * EPS
    # ... and dR/dt there against a central difference over 0.5 ns (truncation (0.0025)^2 |rv|^3 / 6 / bin < 1e-6)
    Rpm = pr.pose(np.array([4100.25, 4100.75]), tab, pos, quat)[1]
    assert pr.max_abs(dR[9], (Rpm[1] - Rpm[0]) / 0.5) < 1e-6 < np.abs(dR[9]).max() * 1e-3


def test_values_equal_the_float64_oracle(adv):
    c = adv["c"]
    p, R = c["pose"][:2]
    o, d = adv["rays"][:2]
    errs = dict(p=pr.max_abs(p, adv["p"].detach().numpy()), R=pr.max_abs(R, adv["R"].detach().numpy()),
                o=pr.max_abs(o, adv["o"].detach().numpy()), d=pr.max_abs(d, adv["d"].detach().numpy()))
    print(errs)
    assert max(errs.values()) < 1e-12, errs


def _first_order(y, ts):
    """d y[i, ...] / d ts[i] by reverse mode, one pass per component (the timestamps are independent)"""
    flat = y.reshape(y.shape[0], -1)
    cols = [torch.autograd.grad(flat[:, k].sum(), ts, retain_graph=True, create_graph=True)[0] for k in range(flat.shape[1])]
    return torch.stack(cols, -1).reshape(y.shape)


def test_first_tangents_equal_autograd_through_the_float64_oracle(adv):
    c = adv["c"]
    bin_ = c["bin"]
    at_first = c["ts"] == float(c["table"][0][0])       # there left == right: both sides give zero, checked below
    got = dict(dp=c["pose"][2], dR=c["pose"][3], do=adv["rays"][2], dd=adv["rays"][3])
    want = dict(dp=_first_order(adv["p"], adv["ts"]), dR=_first_order(adv["R"], adv["ts"]),
                do=_first_order(adv["o"], adv["ts"]), dd=_first_order(adv["d"], adv["ts"]))
    for k in got:
        w = want[k].detach().numpy()
        assert np.isfinite(w).all(), k
        s = bin_.reshape((-1,) + (1,) * (w.ndim - 1))
        err, scale = pr.max_abs(got[k] * s, w * s), float(np.abs(w * s).max())
        print(k, err, scale)
        assert err < 1e-12 * max(scale, 1.0), (k, err)
        assert at_first.sum() >= 1 and (got[k][at_first] == 0).all() and (w[at_first] == 0).all(), k


# Second derivatives against central differences, per unit of the interpolation weight w.  Inside a segment
# g(w) = dR/dw = R(w) S with S = [rv]_x constant, so g'' = R S^3, g''' = R S^4, and the central difference
#     D(w) = (g(w + h) - g(w - h)) / (2 h) = g'(w) + h^2 / 6 g'''(w) + O(h^4):
# every entry of R S^4 is at most |rv|^4 (R orthogonal up to 1e-7, |S x| <= |rv| |x|), so the truncation error is at most
# h^2 |rv|^4 / 6 (+ a relative h^2 |rv|^2 / 20 of it from the next term: 1.01 covers it).  Round-off: rv does not depend on w, only R
# does; an entry of R carries a few EPS of absolute error, so an entry of g a few EPS |rv|, and the difference of two such
# divided by 2 h at most C_ROUND EPS |rv| / h with C_ROUND = 16 (a dozen float64 operations per entry, generously).  The same
# two terms bound the ray direction: d(w) = R(w) k / |k| for a unit quaternion, a unit vector turned by the same rotation.
# h = 2^-16 balances the two at the largest angle: h^2 pi^4 / 6 = 3.8e-9 against 16 EPS pi / h = 7.3e-10; a smaller h buys
# nothing.  The table starts at t = 0 here so that w + h, w - h and w are exact doubles (bins are multiples of 2^10 ns and the
# weights dyadic: every timestamp is a multiple of 2^-6 ns below 2^31 ns) and both stencil points lie inside the segment.
FD_H = 2.0 ** -16
FD_W = (2.0 ** -10, 0.25, 0.5, 0.75, 1 - 2.0 ** -10)
C_ROUND = 16


def _fd_bound(rv_norm):
    return 1.01 * FD_H ** 2 * rv_norm ** 4 / 6 + C_ROUND * EPS * rv_norm / FD_H


@pytest.fixture(scope="module")
def fd():
    table = pr.adversarial_table(t0=0)
    mid, lo, hi = (pr.segment_queries(table[0], ws=[w + s * FD_H for w in FD_W])[1:] for s in (0, -1, 1))
    terms = pr.pose_terms(mid, *table)
    for q in (lo, hi):                                                               # the stencil is exact and in the segment
        tq = pr.pose_terms(q, *table)
        assert (tq["left"] == terms["left"]).all() and (np.abs(tq["w64"] - terms["w64"]) == FD_H).all()
    px = pr.pixels(len(mid))
    return dict(table=table, ts=(lo, mid, hi), terms=terms, px=px)


def test_second_derivatives_equal_central_differences_of_the_first(fd):
    table, (lo, mid, hi), terms, px = fd["table"], fd["ts"], fd["terms"], fd["px"]
    bin_ = terms["bin"]
    rvn = np.linalg.norm(terms["rv"], axis=-1)
    pose_at = {k: pr.pose(q, *table) for k, q in (("lo", lo), ("mid", mid), ("hi", hi))}
    rays_at = {k: pr.rays(pr.KINV_SKEW, px, *v) for k, v in pose_at.items()}
    dw = 2 * FD_H
    fd_ddR = (pose_at["hi"][3] - pose_at["lo"][3]) * bin_[:, None, None] / dw
    fd_ddd = (rays_at["hi"][3] - rays_at["lo"][3]) * bin_[:, None] / dw
    fd_ddp = (pose_at["hi"][2] - pose_at["lo"][2]) * bin_[:, None] / dw
    err_R = np.abs(pose_at["mid"][4] * bin_[:, None, None] ** 2 - fd_ddR).max(axis=(1, 2))
    err_d = np.abs(rays_at["mid"][4] * bin_[:, None] ** 2 - fd_ddd).max(axis=1)
    bound = _fd_bound(rvn)
    nz = bound > 0
    print("worst ddR", (err_R[nz] / bound[nz]).max(), "worst ddd", (err_d[nz] / bound[nz]).max(), "largest bound", bound.max())
    assert (fd_ddp == 0).all()                                                       # p'' = 0: dp/dt is constant in a segment
    assert (err_R <= bound).all() and (err_d <= bound).all()
    assert bound.max() < 5e-9 and np.abs(pose_at["mid"][4] * bin_[:, None, None] ** 2).max() > 9


def test_second_derivatives_equal_double_backward_where_it_is_finite(fd):
    """torch's double backward through the oracle is NaN where a norm or an atan2 is differentiated twice at zero (the 0 rad
    segments, w = 0), which is why the closed form and not autograd is the second-order reference; where it is finite the two agree"""
    table, (_, mid, _), terms, px = fd["table"], fd["ts"], fd["terms"], fd["px"]
    ts = t64(mid).requires_grad_()
    p, R = otraj.linear_trajectory(ts, *(t64(a) for a in table))
    _, d = otraj.pixel_params_to_ray(t64(pr.KINV_SKEW), t64(px), p, R)
    ref = pr.pose(mid, *table)
    ref_rays = pr.rays(pr.KINV_SKEW, px, *ref)
    bin_ = terms["bin"]
    for name, y, want in (("ddR", R, ref[4]), ("ddd", d, ref_rays[4])):
        second = _first_order(_first_order(y, ts), ts).detach().numpy()
        s = (bin_ ** 2).reshape((-1,) + (1,) * (want.ndim - 1))
        finite = np.isfinite(second).reshape(len(mid), -1).all(-1)
        nonzero = np.linalg.norm(terms["rv"], axis=-1) > 0
        print(name, "finite rows", int(finite.sum()), "of", len(mid))
        assert finite[nonzero].all()
        err = pr.max_abs((second * s)[finite], (want * s)[finite])
        assert err < 1e-11 * float(np.abs(want * s).max()), (name, err)


def test_recorded_yardsticks_are_what_the_reference_measures():
    """the constants tests/test_gpu_pose.py takes its bounds from are float32-against-float64 figures of the reference alone;
    measured again here (numpy's float32 sin / cos / atan2 may differ in the last bit between CPUs, hence the 1.5)"""
    import test_gpu_pose as tg
    live = pr.yardsticks()
    assert set(live) == set(tg.YARDSTICK)
    for name, qs in live.items():
        assert set(qs) == set(tg.YARDSTICK[name]), name
        for q, v in qs.items():
            rec = tg.YARDSTICK[name][q]
            assert rec / 1.5 <= v <= rec * 1.5, (name, q, v, rec)
            assert tg.BOUND[name][q] == 4 * rec
    for name in ("adversarial", "outside", "two_knots", "random_1025", "orbit_knots"):       # today's 1e-5 of the largest value
        p, R = pr.case(name)["pose"][:2]
        assert tg.BOUND[name]["p"] <= 1e-5 * np.abs(p).max() and tg.BOUND[name]["R"] <= 1e-5 * np.abs(R).max()
    assert tg.BOUND["raygen"]["d"] <= 1e-5 and tg.BOUND["pose_rays"]["d"] <= 1e-5 and tg.BOUND["pose_rays"]["o"] <= 1e-5 * 6

"""numpy reference of pose interpolation and ray generation with first and second time derivatives, written from the
definitions (oracle/trajectory.py states the value semantics; the derivatives are the closed forms below), generic in the
floating-point type: every operation after the interpolation weight is rounded to `dtype`.  At float64 it is the reference
the pose kernels are held to (tests/test_gpu_pose.py); at float32, on the same inputs, its distance from the float64
evaluation is the yardstick for what a float32 implementation of this chain can deliver.  tests/test_pose_reference_cpu.py
checks it against the oracle, torch autograd and finite differences.  Plus the tables and queries both test files use.

Definitions.  Quaternions are XYZW.  With knots tab_ts[0] < ... < tab_ts[C-1] [ns, int64] and a timestamp t [float64]:

  segment   right = first index with tab_ts[right] >= t (searchsorted, left side); left = right - 1, except at
            t == tab_ts[0], where left = right = 0.  A timestamp on an interior knot k is therefore the END of segment
            k - 1 (w = 1), never the start of segment k.
  OUTSIDE THE TABLE (the reference project asserts this away; the kernels define it, and so does this function):
            t < tab_ts[0]:    left = right = 0 -- the first pose is held, every time derivative is zero;
            t > tab_ts[C-1]:  left = C - 2, right = C - 1 -- the last segment is extrapolated (w > 1).
  weight    bin = tab_ts[s + 1] - tab_ts[s] with s = min(left, C - 2);  w = (t - tab_ts[left]) / bin formed in float64 and
            THEN rounded to dtype;  dw/dt = 1 / bin likewise.
  position  p = lerp(p_l, p_r, w) in torch.lerp's two-sided form (|w| < 0.5: p_l + w (p_r - p_l), else
            p_r - (p_r - p_l)(1 - w));  dp/dt = (p_r - p_l) / bin;  d2p/dt2 = 0.
  rotation  q_r is negated if q_l . q_r < 0 (shortest path);  rel = conj(q_l) (x) q_r;  rv = the full rotation vector of rel
            (angle = 2 atan2(|rel.xyz|, rel.w), rv = rel.xyz * angle / sin(angle / 2), Taylor series at |angle| <= 1e-3);
            q(w) = q_l (x) exp(w rv / 2) (sin(th / 2) / th by its Taylor series at th = |w rv| <= 1e-3);  R = the rotation
            matrix of q(w) WITHOUT normalising q.  Inside a segment R(w) = R(0) exp(w [rv]_x), hence
            dR/dt = R [rv]_x / bin   and   d2R/dt2 = R [rv]_x^2 / bin^2.
  rays      m = R K^-1 [u v 1]^T, o = p, d = m / |m|; with n = |m|, n' = d . m', n'' = (m'.m' + m.m'' - n'^2) / n:
            d' = (m' - d n') / n,   d'' = (m'' - 2 d' n' - d n'') / n      (quotient rule on d n = m, twice).
"""
import numpy as np

SMALL_ANGLE = 1e-3


# ------------------------------------------------------------------------------------------------ quaternions (XYZW)
def _qmul(p, q):
    pv, pw, qv, qw = p[..., :3], p[..., 3:], q[..., :3], q[..., 3:]
    v = pw * qv + qw * pv + np.cross(pv, qv)
    w = pw * qw - (pv * qv).sum(-1, keepdims=True)
    return np.concatenate([v, w], -1)


def _qconj(q):
    return np.concatenate([-q[..., :3], q[..., 3:]], -1)


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _full_rotvec(q, dt):
    """unit quaternion -> rotation vector with angle in [0, 2 pi]; also the angle"""
    angle = dt(2) * np.arctan2(_norm(q[..., :3]), q[..., 3])
    small = np.abs(angle) <= dt(SMALL_ANGLE)
    a2 = angle * angle
    safe = np.where(small, dt(1), angle)
    scale = np.where(small, dt(2) + a2 / dt(12) + dt(7) * a2 * a2 / dt(2880), safe / np.sin(safe / dt(2)))
    return scale[..., None] * q[..., :3], angle


def _exp_quat(r, dt):
    """rotation vector -> unit quaternion"""
    th = _norm(r)
    small = th <= dt(SMALL_ANGLE)
    t2 = th * th
    safe = np.where(small, dt(1), th)
    s = np.where(small, dt(0.5) - t2 / dt(48) + t2 * t2 / dt(3840), np.sin(safe / dt(2)) / safe)
    return np.concatenate([s[..., None] * r, np.cos(th / dt(2))[..., None]], -1)


def _rotmat(q):
    x, y, z, w = (q[..., k] for k in range(4))
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.stack([x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw),
                  2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw),
                  2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2], -1)
    return m.reshape(*q.shape[:-1], 3, 3)


def _skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], -1).reshape(
        *v.shape[:-1], 3, 3)


def _matmul(a, b):
    """batched 3x3 (or 3x3 by 3) product with every term in the arrays' own type"""
    if b.ndim == a.ndim:
        return (a[..., :, :, None] * b[..., None, :, :]).sum(-2)
    return (a * b[..., None, :]).sum(-1)


# ------------------------------------------------------------------------------------------------ pose
def segments(ts, tab_ts):
    """-> left, right (int64), bin [ns, float64] per timestamp: the segment rule of the module docstring"""
    ts = np.asarray(ts, np.float64)
    tab = np.asarray(tab_ts, np.int64).astype(np.float64)
    C = len(tab)
    assert C >= 2
    right = np.searchsorted(tab, ts, side="left")
    left = np.where(ts == tab[0], right, right - 1)
    before, after = ts < tab[0], ts > tab[-1]
    left, right = np.where(before, 0, left), np.where(before, 0, right)              # hold the first pose
    left, right = np.where(after, C - 2, left), np.where(after, C - 1, right)        # extrapolate the last segment
    s = np.minimum(left, C - 2)
    return left, right, tab[s + 1] - tab[s]


def pose_terms(ts, tab_ts, tab_pos, tab_quat, dtype=np.float64):
    """every intermediate of the chain, by name, rounded to dtype (left, right, bin, w64 excepted)"""
    dt = np.dtype(dtype).type
    ts = np.asarray(ts, np.float64)
    left, right, bin_ = segments(ts, tab_ts)
    w64 = (ts - np.asarray(tab_ts, np.int64).astype(np.float64)[left]) / bin_
    w, wdot = w64.astype(dt), (1.0 / bin_).astype(dt)
    pos, quat = np.asarray(tab_pos).astype(dt), np.asarray(tab_quat).astype(dt)
    a, b = pos[left], pos[right]
    wc = w[:, None]
    p = np.where(np.abs(wc) < dt(0.5), a + wc * (b - a), b - (b - a) * (dt(1) - wc))
    dp = (b - a) * wdot[:, None]
    q0, q1 = quat[left], quat[right]
    dot = (q0 * q1).sum(-1, keepdims=True)
    q1 = np.where(dot < 0, -q1, q1)
    rel = _qmul(_qconj(q0), q1)
    rv, angle = _full_rotvec(rel, dt)
    q = _qmul(q0, _exp_quat(wc * rv, dt))
    R = _rotmat(q)
    S = _skew(rv)
    dR_dw = _matmul(R, S)
    ddR_dw = _matmul(dR_dw, S)
    out = dict(left=left, right=right, bin=bin_, w64=w64, w=w, wdot=wdot, dot=dot[:, 0], rel=rel, angle=angle, rv=rv, q=q,
               p=p, R=R, dp=dp, dR=dR_dw * wdot[:, None, None], ddR=ddR_dw * (wdot * wdot)[:, None, None])
    for k in ("w", "wdot", "rel", "angle", "rv", "q", "p", "R", "dp", "dR", "ddR"):
        assert out[k].dtype == dt, k
    return out


def pose(ts, tab_ts, tab_pos, tab_quat, dtype=np.float64):
    """ts (B,) float64 [ns], tab_ts (C,) int64, tab_pos (C, 3), tab_quat (C, 4) XYZW -> p (B, 3), R (B, 3, 3), dp/dt (B, 3),
    dR/dt (B, 3, 3), d2R/dt2 (B, 3, 3) per ns, in dtype.  Timestamps outside the table: the first pose is held with zero
    derivatives before tab_ts[0], the last segment is extrapolated after tab_ts[-1] (module docstring)."""
    t = pose_terms(ts, tab_ts, tab_pos, tab_quat, dtype)
    return t["p"], t["R"], t["dp"], t["dR"], t["ddR"]


def rays(Kinv, px, p, R, dp=None, dR=None, ddR=None, dtype=np.float64):
    """Kinv (3, 3), px (B, 2) pixel (u, v), pose and its time derivatives -> o, d, do/dt, dd/dt, d2d/dt2, each (B, 3);
    derivatives that are not given count as zero"""
    dt = np.dtype(dtype).type
    Kinv, px, p, R = (np.asarray(a).astype(dt) for a in (Kinv, px, p, R))
    zero3, zero33 = np.zeros_like(p), np.zeros_like(R)
    dp, dR, ddR = (z if a is None else np.asarray(a).astype(dt) for a, z in ((dp, zero3), (dR, zero33), (ddR, zero33)))
    hom = np.concatenate([px, np.ones_like(px[:, :1])], -1)
    k = _matmul(Kinv[None], hom)
    m, m1, m2 = _matmul(R, k), _matmul(dR, k), _matmul(ddR, k)
    n = _norm(m)[:, None]
    d = m / n
    n1 = (d * m1).sum(-1, keepdims=True)
    n2 = ((m1 * m1).sum(-1, keepdims=True) + (m * m2).sum(-1, keepdims=True) - n1 * n1) / n
    d1 = (m1 - d * n1) / n
    d2 = (m2 - dt(2) * d1 * n1 - d * n2) / n
    for v in (d, d1, d2):
        assert v.dtype == dt
    return p, d, dp, d1, d2


# ------------------------------------------------------------------------------------------------ tables and queries
T0_REAL = int(round(1.7e18 / 1024)) * 1024            # a timestamp of real size [ns]: a double resolves 256 ns there
ADVERSARIAL_ANGLES = (0.0, 1e-6, 3e-4, 9.99e-4, 1.001e-3, 5e-3, 0.05, 0.7, 2.0, 3.0, 3.1, 1e-3, 0.3, 0.0, 2.5)
ONE_TICK_SEGMENT = 12                                 # the 0.3 rad segment is exactly 1024 ns wide
QUERY_W = (1e-7, 1e-3, 0.25, 0.4999, 0.5, 0.5001, 0.75, 0.999, 1.0)
MIN_ABS_DOT = 0.02


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _chain(q0, angles, rng):
    """float32 quaternions q[k + 1] = q[k] (x) exp(angle[k] axis[k] / 2), random axes; an angle of 0 repeats q[k] exactly"""
    q = [np.float32(q0)]
    for a in angles:
        axis = _unit(rng.standard_normal(3))
        step = np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])
        q.append(q[-1] if a == 0.0 else _qmul(q[-1].astype(np.float64), step).astype(np.float32))
    return np.stack(q)


def adversarial_table(t0=T0_REAL, seed=7):
    """16 knots: the relative angles above about random axes, every third quaternion negated, knot times t0 + cumulative
    widths of 1024 * U{1..40000} ns (one bin exactly 1024 ns), positions N(0, 3^2) -> tab_ts int64, tab_pos, tab_quat f32"""
    rng = np.random.default_rng(seed)
    quat = _chain(_unit(rng.standard_normal(4)), ADVERSARIAL_ANGLES, rng)
    quat[::3] *= -1
    widths = 1024 * rng.integers(1, 40001, size=len(ADVERSARIAL_ANGLES))
    widths[ONE_TICK_SEGMENT] = 1024
    tab_ts = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64) + np.int64(t0)
    tab_pos = (3.0 * rng.standard_normal((len(quat), 3))).astype(np.float32)
    return tab_ts, tab_pos, quat.astype(np.float32)


def random_table(C, seed, t0=T0_REAL):
    """C knots with independent random unit quaternions (so half the neighbours need the flip); a quaternion closer than
    MIN_ABS_DOT to perpendicular to its predecessor is drawn again"""
    rng = np.random.default_rng(seed)
    quat = np.empty((C, 4), np.float32)
    for k in range(C):
        while True:
            quat[k] = _unit(rng.standard_normal(4)).astype(np.float32)
            if k == 0 or abs(float(quat[k].astype(np.float64) @ quat[k - 1].astype(np.float64))) >= MIN_ABS_DOT:
                break
    widths = 1024 * rng.integers(1, 40001, size=C - 1)
    tab_ts = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64) + np.int64(t0)
    return tab_ts, (3.0 * rng.standard_normal((C, 3))).astype(np.float32), quat


def min_abs_dot(tab_quat):
    q = np.asarray(tab_quat, np.float64)
    return float(np.abs((q[:-1] * q[1:]).sum(-1)).min())


def segment_queries(tab_ts, ws=QUERY_W, segs=None):
    """tab_ts[k] + w * width in float64 for every segment k (or those in segs) and w in ws, and w = 0 on the first segment"""
    tab = np.asarray(tab_ts, np.int64)
    segs = range(len(tab) - 1) if segs is None else segs
    out = [float(tab[0])] if 0 in segs else []
    for k in segs:
        width = float(tab[k + 1] - tab[k])
        out += [float(tab[k]) + w * width for w in ws]
    return np.array(out, np.float64)


def outside_queries(tab_ts):
    """timestamps up to 1.5 bins before the first knot and after the last one (multiples of 1024 ns from the ends)"""
    tab = np.asarray(tab_ts, np.int64)
    first, last = int(tab[1] - tab[0]) // 1024, int(tab[-1] - tab[-2]) // 1024
    before = [float(tab[0] - 1024 * max(1, int(f * first))) for f in (0.0, 0.3, 0.5, 1.0, 1.5)]
    after = [float(tab[-1] + 1024 * max(1, int(f * last))) for f in (0.0, 0.3, 0.5, 1.0, 1.5)]
    return np.array(before, np.float64), np.array(after, np.float64)


SENSOR_W, SENSOR_H = 346, 260
KINV_SKEW = np.linalg.inv(np.array([[290.0, 1.7, 172.3], [0.0, 288.5, 131.9], [0.0, 0.0, 1.0]])).astype(np.float32)


def pixels(n, seed=3):
    """(n, 2) float32 pixel positions of a 346 x 260 sensor: the principal point of KINV_SKEW's camera, the four image
    corners, then random pixels"""
    rng = np.random.default_rng(seed)
    fixed = [(172.3, 131.9), (0, 0), (SENSOR_W - 1, 0), (0, SENSOR_H - 1), (SENSOR_W - 1, SENSOR_H - 1)]
    rnd = np.stack([rng.integers(0, SENSOR_W, size=n), rng.integers(0, SENSOR_H, size=n)], -1)
    return np.concatenate([np.array(fixed, np.float64), rnd.astype(np.float64)])[:n].astype(np.float32)


def max_abs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.size(a) else 0.0


def pose_errors(got, want, bin_):
    """max absolute error per quantity of a pose 5-tuple (or a prefix of one) against `want`; time derivatives are compared
    per unit of the interpolation weight: first ones times bin, second ones times bin^2"""
    names, power = ("p", "R", "dp", "dR", "ddR"), (0, 0, 1, 1, 2)
    out = {}
    for name, pw, g, w in zip(names, power, got, want):
        if g is None:
            continue
        s = np.asarray(bin_, np.float64) ** pw
        s = s.reshape((-1,) + (1,) * (np.ndim(w) - 1))
        out[name] = max_abs(np.asarray(g, np.float64) * s, np.asarray(w, np.float64) * s)
    return out


def ray_errors(got, want, bin_):
    """the same for a ray 5-tuple o, d, do, dd, ddd"""
    names, power = ("o", "d", "do", "dd", "ddd"), (0, 0, 1, 1, 2)
    out = {}
    for name, pw, g, w in zip(names, power, got, want):
        if g is None:
            continue
        s = (np.asarray(bin_, np.float64) ** pw)[:, None]
        out[name] = max_abs(np.asarray(g, np.float64) * s, np.asarray(w, np.float64) * s)
    return out


# ------------------------------------------------------------------------------------------------ the cases of both test files
CASES = ("adversarial", "outside", "two_knots", "random_1025", "orbit_knots")
_case_cache = {}


def case(name):
    """-> dict(table=(tab_ts, tab_pos, tab_quat), ts, bin, pose=float64 pose 5-tuple), computed once and read-only"""
    if name in _case_cache:
        return _case_cache[name]
    if name == "adversarial":
        table = adversarial_table()
        ts = segment_queries(table[0])
    elif name == "outside":
        table = adversarial_table()
        ts = np.concatenate(outside_queries(table[0]))
    elif name == "two_knots":
        table = random_table(2, seed=11)
        ts = segment_queries(table[0])
    elif name == "random_1025":                   # 11 levels of binary search; both ends, the middle and random segments
        table = random_table(1025, seed=12)
        segs = sorted({0, 1, 511, 512, 513, 1022, 1023} | set(np.random.default_rng(5).integers(0, 1024, 40).tolist()))
        ts = segment_queries(table[0], segs=segs)
    elif name == "orbit_knots":                   # the smooth arc of tests/golden/trajectory.npz, queried on every knot
        import os
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory.npz"))
        table = (g["tab_ts"], g["tab_pos"], g["tab_quat"])
        ts = g["tab_ts"].astype(np.float64)
    else:
        raise KeyError(name)
    c = dict(table=table, ts=ts, bin=segments(ts, table[0])[2], pose=pose(ts, *table))
    for a in (*table, ts, c["bin"], *c["pose"]):
        a.setflags(write=False)
    _case_cache[name] = c
    return c


def tiled(a, n):
    """the first n rows of a repeated cyclically"""
    return a[np.arange(n) % len(a)]


def ray_inputs(name="adversarial"):
    """what a ray generator is handed: the float64 pose of a case rounded to float32, with that case's bin and pixels"""
    c = case(name)
    return tuple(a.astype(np.float32) for a in c["pose"]), c["bin"], pixels(len(c["ts"]))


POSE_RAYS_LAYOUTS = ((136, 136), (272, 136), (257, 1), (257, 100))          # (R, px_rows)


def pose_rays_case(R, px_rows, dtype=np.float64):
    """timestamps (the adversarial queries, cyclically), pixels and the rays o, d of pixel i % px_rows at the pose of ts[i]"""
    c = case("adversarial")
    ts, px = tiled(c["ts"], R), pixels(px_rows)
    p, Rm = pose(ts, *c["table"], dtype=dtype)[:2]
    o, d = rays(KINV_SKEW, tiled(px, R), p, Rm, dtype=dtype)[:2]
    return ts, px, (o, d)


def yardsticks():
    """max |float32 evaluation - float64 evaluation| of this module on the same inputs, per case and quantity: what
    tests/test_gpu_pose.py records as YARDSTICK"""
    out = {}
    for name in CASES:
        c = case(name)
        out[name] = pose_errors(pose(c["ts"], *c["table"], dtype=np.float32), c["pose"], c["bin"])
    f32, bin_, px = ray_inputs()
    out["raygen"] = ray_errors(rays(KINV_SKEW, px, *f32, dtype=np.float32), rays(KINV_SKEW, px, *f32), bin_)
    worst = {"o": 0.0, "d": 0.0}
    for R, rows in POSE_RAYS_LAYOUTS:
        e = ray_errors(pose_rays_case(R, rows, np.float32)[2], pose_rays_case(R, rows)[2], np.ones(R))
        worst = {k: max(worst[k], e[k]) for k in worst}
    out["pose_rays"] = worst
    return out

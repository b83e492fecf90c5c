"""numpy restatement of the depth-map fusion (include/ren_amd.h "tsdf"), written from the specification and not from the
kernel: float32 arrays and one numpy operation per listed operation, so nothing fuses; float64 for the lattice positions; a
loop over the views; integer counts.  The GPU tests hold the kernel to it bit for bit.

Also a small analytic depth renderer (z-depth of a sphere from a pinhole camera, +inf off the sphere), the camera rings and
the measurement that tests/test_tsdf_cpu.py and tests/test_gpu_tsdf.py share.
"""
import numpy as np

F = np.float32


def lattice_axes(lo, hi, res):
    """per axis the float32 coordinates float32(lo + double(idx) * step), step = (hi - lo) / (n - 1) in float64"""
    axes = []
    for a in range(3):
        step = (np.float64(hi[a]) - np.float64(lo[a])) / np.float64(res[a] - 1)
        prod = np.arange(res[a], dtype=np.float64) * step
        axes.append((np.float64(lo[a]) + prod).astype(F))
    return axes


def lattice(lo, hi, res):
    """(n, 3) float32 in linear index order p = (i * ny + j) * nz + k"""
    x, y, z = np.meshgrid(*lattice_axes(lo, hi, res), indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)


def integrate(depth, cams, K, lo, hi, res, trunc, z_min, total, count):
    """steps 1 - 11 of the header for depth (V, H, W), cams (V, 12), K 3 x 3: total (n,) float32 and count (n,) int32 are
    updated in place, the views in ascending order"""
    depth, cams, K = np.asarray(depth, dtype=F), np.asarray(cams, dtype=F), np.asarray(K, dtype=F)
    n_views, height, width = depth.shape
    assert cams.shape == (n_views, 12) and total.dtype == F and count.dtype == np.int32
    trunc, z_min = F(trunc), F(z_min)
    k00, k01, k02, k11, k12 = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    x = lattice(lo, hi, res)                                                         # 1
    with np.errstate(all="ignore"):
        for v in range(n_views):
            c, R = cams[v, :3], cams[v, 3:].reshape(3, 3)
            d = [x[:, a] - c[a] for a in range(3)]                                   # 2
            q = []
            for a in range(3):                                                       # 3
                m0 = R[0, a] * d[0]
                m1 = R[1, a] * d[1]
                m2 = R[2, a] * d[2]
                s01 = m0 + m1
                q.append(s01 + m2)
            z = q[2]                                                                 # 4
            ok = z > z_min
            xn = q[0] / z                                                            # 5
            yn = q[1] / z
            a0 = k00 * xn                                                            # 6
            a1 = k01 * yn
            a01 = a0 + a1
            u = a01 + k02
            b1 = k11 * yn
            w = b1 + k12
            fu = np.floor(u + F(0.5))                                                # 7
            fv = np.floor(w + F(0.5))
            assert fu.dtype == F and fv.dtype == F and z.dtype == F
            ok &= (fu >= 0) & (fu < F(width)) & (fv >= 0) & (fv < F(height))
            iu = np.where(ok, fu, 0).astype(np.int64)
            iv = np.where(ok, fv, 0).astype(np.int64)
            if height * width:
                D = depth[v].reshape(-1)[iv * width + iu]                            # 8
            else:
                D = np.full(len(z), np.nan, dtype=F)
            ok &= ~(np.isnan(D) | (D <= 0))
            s = D - z                                                                # 9
            ok &= ~(s < -trunc)
            t = np.where(s >= trunc, F(1.0), s / trunc)                              # 10
            assert t.dtype == F
            total[ok] = total[ok] + t[ok]                                            # 11
            count[ok] += 1


def fuse(depth, cams, K, lo, hi, res, trunc, z_min=1e-6, state=None):
    """-> field (nx, ny, nz) float32 (-(sum / count) where count > 0, else -1), count (nx, ny, nz) int32, state = (sum, count)
    flat, continued in place by a further call"""
    n = res[0] * res[1] * res[2]
    if state is None:
        state = (np.zeros(n, dtype=F), np.zeros(n, dtype=np.int32))
    total, count = state
    integrate(depth, cams, K, lo, hi, res, trunc, z_min, total, count)
    with np.errstate(all="ignore"):
        mean = total / count.astype(F)
    field = np.where(count > 0, -mean, F(-1.0)).astype(F)
    return field.reshape(res), count.reshape(res).copy(), state


# ---- cameras and the analytic renderer ------------------------------------------------------------------------------------
def look_at(centre, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """camera-to-world rotation (float64) whose column 2 looks from `centre` to `target`; column 0 right, column 1 down"""
    c, t = np.asarray(centre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (t - c) / np.linalg.norm(t - c)
    right = np.cross(fwd, np.asarray(up, dtype=np.float64))
    if np.linalg.norm(right) < 1e-9:
        right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.stack([right, down, fwd], axis=1)


def pack(centres, rots):
    """(V, 12) float32: centre, then the rotation row-major"""
    return np.concatenate([np.asarray(centres, dtype=np.float64).reshape(-1, 3), np.asarray(rots, dtype=np.float64).reshape(-1, 9)],
                          axis=1).astype(F)


def pinhole(f, height, width):
    return np.array([[f, 0.0, (width - 1) / 2.0], [0.0, f, (height - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=F)


def sphere_depth(cams, K, height, width, radius, centre=(0.0, 0.0, 0.0)):
    """(V, H, W) float32: z-depth of the sphere through the centre of every pixel (float64 geometry), +inf off the sphere"""
    K = np.asarray(K, dtype=np.float64)
    xs, ys = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64), indexing="xy")
    yn = (ys - K[1, 2]) / K[1, 1]
    xn = (xs - K[0, 2] - K[0, 1] * yn) / K[0, 0]
    out = np.full((len(cams), height, width), np.inf, dtype=F)
    for v, cam in enumerate(np.asarray(cams, dtype=np.float64)):
        c, R = cam[:3], cam[3:].reshape(3, 3)
        d = np.stack([xn, yn, np.ones_like(xn)], axis=-1) @ R.T                      # world direction with unit z-depth per unit t
        oc = c - np.asarray(centre, dtype=np.float64)
        a, b, cc = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - radius * radius
        disc = b * b - 4.0 * a * cc
        with np.errstate(invalid="ignore"):
            t = (-b - np.sqrt(disc)) / (2.0 * a)
        hit = (disc >= 0) & (t > 0)
        out[v][hit] = t[hit].astype(F)
    return out


def two_rings(n=12, distance=2.0, heights=(0.5, -0.5)):
    """n cameras on two rings at `distance` from the origin, at z = +-heights * distance / |.|, looking at the origin"""
    centres = []
    per = n // len(heights)
    for r, h in enumerate(heights):
        for k in range(per):
            phi = 2.0 * np.pi * (k + 0.5 * r) / per
            rho = np.sqrt(1.0 - h * h)
            centres.append(distance * np.array([rho * np.cos(phi), rho * np.sin(phi), h]))
    return pack(centres, [look_at(c) for c in centres])


# ---- the sphere set-up both test files use ---------------------------------------------------------------------------------
SPHERE = dict(radius=0.5, res=(33, 33, 33), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), height=64, width=64, f=64.0)
SPHERE["spacing"] = 2.0 / 32
SPHERE["trunc"] = 3 * SPHERE["spacing"]
# mean and maximum of | |vertex| - 0.5 | over the outer surface, measured with this file alone (test_tsdf_cpu.py prints them;
# DESIGN 3.15): the bounds of both test files derive from the spacing and from MEASURED_MAX
MEASURED_MEAN, MEASURED_MAX = 0.009747, 0.049459


def sphere_inputs():
    cams = two_rings()
    K = pinhole(SPHERE["f"], SPHERE["height"], SPHERE["width"])
    return sphere_depth(cams, K, SPHERE["height"], SPHERE["width"], SPHERE["radius"]), cams, K


def fill_inner_shell(field):
    """the outside points (field < 0) with |x| < radius - trunc / 2 set to +1: what mesh.clean(fill_cavities=True) does to the
    cavity the inner shell bounds.  (Filling only |x| < radius - trunc - spacing would leave the never-seen points between
    that radius and the shell outside, and with them a surface around the filled ball.)"""
    x = lattice(SPHERE["lo"], SPHERE["hi"], SPHERE["res"]).astype(np.float64)
    out = field.copy().reshape(-1)
    inner = (np.linalg.norm(x, axis=1) < SPHERE["radius"] - SPHERE["trunc"] / 2) & (out < 0)
    out[inner] = 1.0
    return out.reshape(field.shape)


def radial_error(verts):
    """-> (mean, max) of | |v| - radius | over the vertices of radius above radius - trunc / 2, and the radii of all"""
    rad = np.linalg.norm(np.asarray(verts, dtype=np.float64), axis=1)
    outer = rad > SPHERE["radius"] - SPHERE["trunc"] / 2
    err = np.abs(rad[outer] - SPHERE["radius"])
    return float(err.mean()), float(err.max()), rad

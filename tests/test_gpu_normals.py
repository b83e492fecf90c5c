"""Surface normals: the one-launch input gradient of the grid encoding (ren_hashgrid_bwd_input, csrc/ren_normals.hip),
Renderer.density_gradient and evaluation.render_normal_image.

The kernel is checked against two independent references:
 (a) the oracle: torch.autograd.grad through oracle.hashgrid.encode (float64 table; float32 positions, for which the oracle
     reproduces fmaf(scale, x, .5) exactly and so selects the kernel's cells), composed with oracle.field.contract;
 (b) the three-launch construction the tcnn seam uses (ren_hashgrid_fwd_jvp with unit tangents, contracted with dfeat):
     the same table reads through different code, with identical float32 cell selection.
The gradient of a trilinear interpolation jumps at cell faces, so (a) is compared element-wise only on the samples at least
2^-20 of a cell from every face at every level (the share left out is asserted < 1 %), and by rel_err on all of them.
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from conftest import field_params_from, load_golden, rel_err, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FACE = 2.0 ** -20                      # of a cell
SIZES = (1, 33, 257, 1000 + 7)         # one lane | crosses a 32-sample fragment | crosses a 256-thread workgroup | ragged tail
N = SIZES[-1]

GRIDS = {
    "hash": dict(),                                                        # levels 5.. hashed, 2^19 entries each
    "dense": dict(otype="DenseGrid", per_level_scale=1.1),                 # res 16 .. 67
    "tiled": dict(otype="TiledGrid"),                                      # 16^3 entries per level, z dropped from res 71 on
}
# the scene form: a small hashed grid (2^14 entries, hashed from res 27 on; finest scale 245) -- the contraction runs in
# float32 on the GPU and on the CPU and the two unit positions differ by an ulp or two; at scale 245 that is < 2^-15 of a cell
SCENE_GRID = dict(log2_hashmap_size=14, per_level_scale=1.2)
SCENES = {"aabb": (0, 101), "tanh": (1, 101), "sphere": (2, 105)}             # contraction type, seed
AABB = [-1.0, -1.5, -0.5, 2.0, 1.5, 1.5]

# Round-off bound against (a), relative to the largest entry: the forward test (test_gpu_grid_types.py) allows 2e-6 for an
# 8-term interpolation; a gradient component is such a sum per level with a two-term dot product (entry . dfeat) inside each
# term, times the level's scale, summed over 16 levels in float32: twice the operations -> 4e-6.  Element-wise (conftest's
# elem_err judges elements below 1e-3 of the scale against that floor) the same absolute error is 4e-6 / 1e-3.
REL_A = 4e-6
ELEM_A = REL_A / 1e-3
# The scene form adds the round-off of the POSITION: the tanh / sphere contraction is a handful of rounded float32 operations
# (tanhf; sqrt, two divisions, a product, an fma), good to about 2 ulps, so the unit position the GPU forms and the one the
# oracle forms differ by up to 4 ulps of a number below 1 (4 x 2^-24).  Inside a cell the gradient is not constant: its
# derivative is scale^2 x (weights of ONE remaining axis) x entries against scale x (weights of TWO axes) x entries, i.e.
# about 2 x scale per unit of position relative to the gradient itself (weights average 1/2), and the finest level (scale 245
# on SCENE_GRID) carries the largest share.  4 x 2^-24 x 2 x 245 = 1.2e-4.  (aabb is two exactly rounded operations and agrees
# bit for bit; it is held to the same bound.)
REL_SCENE = REL_A + 4 * 2.0 ** -24 * 2 * 245
ELEM_SCENE = REL_SCENE / 1e-3


def dev(x):
    return torch.as_tensor(x).to(DEV).contiguous()


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import engine, ops, _lib
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, engine


def to_frag(rows):
    n = rows.shape[0]
    nb = (n + 31) // 32
    pad = torch.zeros(nb * 32, 32, dtype=torch.float32)
    pad[:n] = rows
    return pad.view(nb, 32, 16, 2).permute(0, 2, 3, 1).contiguous().view(-1)


def face_distance(xu, spec):
    """(n,) smallest distance, in cells, of the float32 level position fmaf(scale, x, .5) from a cell face, over the levels
    and the three coordinates; and the same in units of the position's float32 ulp"""
    dist = torch.full((xu.shape[0],), float("inf"), dtype=torch.float64)
    ulps = dist.clone()
    for s in spec.scales:
        pos = (xu.detach().double() * float(s) + 0.5).float().double()
        dd = (pos - torch.round(pos)).abs()
        ulp = torch.from_numpy(np.spacing(pos.abs().clamp(min=1.0).float().numpy())).double()
        dist = torch.minimum(dist, dd.min(dim=1).values)
        ulps = torch.minimum(ulps, (dd / ulp).min(dim=1).values)
    return dist, ulps


def unit_points(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, generator=g)
    x[1:9] = torch.tensor([[0.0, 0.31, 0.69], [1.0, 0.62, 0.23], [0.41, 0.0, 0.93], [0.83, 1.0, 0.13],
                           [0.55, 0.45, 0.0], [0.35, 0.65, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])    # on the box faces
    x[9:17] = x[1:9] + (x[1:9] - 0.5).sign() * 1e-3 * (x[1:9] - 0.5).abs().ge(0.5)                # ... and just outside them
    x[17:33] = torch.rand(16, 3, generator=g) * 1.4 - 0.2                                           # well outside
    return x.contiguous()


_CACHE = {}


def unit_case(name):
    """inputs and reference (a) of one grid type, computed once: x (N, 3) unit cube, dfeat (N, 32), table of order 1"""
    if name not in _CACHE:
        from oracle import hashgrid
        spec = hashgrid.make_spec(**GRIDS[name])
        table = hashgrid.init_table(spec, 11, 1.0, "mix32")
        x = unit_points(3)
        g = torch.Generator().manual_seed(4)
        dfeat = torch.randn(N, 32, generator=g)
        xr = x.clone().requires_grad_()
        enc = hashgrid.encode(xr, table.double(), spec)
        (ref,) = torch.autograd.grad((enc * dfeat.double()).sum(), xr)
        dist, _ = face_distance(x, spec)
        _CACHE[name] = dict(spec=spec, table=table, x=x, dfeat=dfeat, ref=ref.double(), safe=dist >= FACE)
    return _CACHE[name]


def jvp3_unit(ops, grid, table_d, x_d, dfeat_rows_d):
    """reference (b), unit-cube form: tcnn_api._encode_with_tangent with the unit tangents"""
    from robust_e_nerf_amd import tcnn_api
    mod = types.SimpleNamespace(grid=grid, unit_scene=ops.make_scene_desc([0, 0, 0, 1, 1, 1], ops.AABB))
    cols = []
    for k in range(3):
        e = torch.zeros_like(x_d)
        e[:, k] = 1.0
        cols.append((tcnn_api._encode_with_tangent(mod, table_d, x_d, e)[1] * dfeat_rows_d).sum(-1))
    return torch.stack(cols, -1)


def jvp3_scene(ops, grid, table_d, scene, o, d, ri, ts, te, dfeat_rows_d):
    """reference (b), scene form: the same three launches over the real rays, the origin's time derivative = e_k"""
    from robust_e_nerf_amd import _lib, tcnn_api
    from robust_e_nerf_amd.ops import _ptr, _stream
    n = ri.shape[0]
    nb = ops.n_blocks32(n)
    zero = torch.zeros_like(o)
    cols = []
    for k in range(3):
        e = torch.zeros_like(o)
        e[:, k] = 1.0
        feat, featd = torch.empty(nb * 1024, device=DEV), torch.empty(nb * 1024, device=DEV)
        _lib.check(_lib.load().ren_hashgrid_fwd_jvp(ctypes.byref(grid), _ptr(table_d), ctypes.byref(scene), _ptr(o), _ptr(d),
                                                    _ptr(e), _ptr(zero), _ptr(ri), _ptr(ts), _ptr(te), n, _ptr(feat),
                                                    _ptr(featd), None, _stream()), "ren_hashgrid_fwd_jvp")
        cols.append((tcnn_api._to_rows(featd, n) * dfeat_rows_d).sum(-1))
    return torch.stack(cols, -1)


def b_error(ref_a, ref_b, safe):
    """(b)'s own error against (a) over the whole input set, relative to the largest entry; and that entry"""
    scale = float(ref_a.abs().max())
    return float((ref_b[safe] - ref_a[safe]).abs().max()) / scale, scale


def check_against_references(got, ref_a, ref_b, safe, e_ba, scale, tag, rel_a=REL_A, elem_a=ELEM_A):
    """the two rules of the module docstring, errors relative to the largest entry of the whole input set"""
    e_kb = float((got - ref_b).abs().max()) / scale                         # every element
    e_ka = float((got - ref_a).abs().max()) / scale                         # rel_err, all samples
    den = ref_a[safe].abs().clamp(min=1e-3 * scale)                         # elem_err, the samples away from the faces
    e_ka_elem = float(((got[safe] - ref_a[safe]).abs() / den).max()) if bool(safe.any()) else 0.0
    print(f"{tag}: kernel vs (b) {e_kb:.2e} [bound 2 x {e_ba:.2e}]  kernel vs (a) rel {e_ka:.2e} elem {e_ka_elem:.2e}  "
          f"left out {int((~safe).sum())} of {safe.numel()}")
    assert e_kb <= 2 * e_ba, (tag, e_kb, e_ba)
    assert e_ka < rel_a and e_ka_elem < elem_a, (tag, e_ka, e_ka_elem)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_bwd_input_unit_cube_vs_oracle_and_jvp(amd, name, layout):
    """dx = J_x^T dfeat in the unit cube, HashGrid / DenseGrid / TiledGrid, both dfeat layouts, n = 1, 33, 257, 1007, points on
    and outside the box faces, table values of order 1.  Bounds: against (b) twice (b)'s own error against (a); against (a)
    REL_A / ELEM_A above.  Nothing past 3n floats of the output is written.
    Measured (MI355X, n = 1007, either layout): (b) vs (a) 2.3e-7 / 2.6e-7 / 1.6e-7 (hash / dense / tiled), kernel vs (b)
    1.7e-7 / 1.4e-7 / 1.3e-7, kernel vs (a) rel 2.3e-7 / 1.9e-7 / 1.9e-7, elem 6.7e-5 / 4.5e-5 / 2.3e-5; 3 / 0 / 3 of 1007
    samples left out."""
    ops, _ = amd
    c = unit_case(name)
    grid, n_params = ops.make_grid_desc(**GRIDS[name])
    assert n_params == c["spec"].n_params
    assert float((~c["safe"]).float().mean()) < 0.01
    td, xd, dd = dev(c["table"]), dev(c["x"]), dev(c["dfeat"])
    ref_b = jvp3_unit(ops, grid, td, xd, dd).cpu().double()
    e_ba, scale = b_error(c["ref"], ref_b, c["safe"])
    for n in SIZES:
        df = dd[:n].contiguous() if layout == 0 else dev(to_frag(c["dfeat"][:n]))
        out = torch.full((n + 5, 3), -7.0, device=DEV)
        ops.hashgrid_bwd_input(grid, td, df, x_unit=xd[:n].contiguous(), n=n, layout=layout, out=out)
        assert bool((out[n:] == -7.0).all()), "wrote past row n"
        check_against_references(out[:n].cpu().double(), c["ref"][:n], ref_b[:n], c["safe"][:n], e_ba, scale,
                                 f"{name} layout {layout} n {n}")


def scene_case(ct_name):
    if ct_name not in _CACHE:
        from oracle import field as ofield, hashgrid
        ct, seed = SCENES[ct_name]
        spec = hashgrid.make_spec(**SCENE_GRID)
        table = hashgrid.init_table(spec, 17, 1.0, "mix32")
        g = torch.Generator().manual_seed(seed)
        R, n = 48, 517
        aabb = torch.tensor(AABB)
        centre, half = (aabb[:3] + aabb[3:]) / 2, (aabb[3:] - aabb[:3]) / 2
        # origins around the box at up to 2.5 half-extents: with the sphere contraction the samples fall inside and outside the
        # unit ball (both branches); with aabb some fall on the far side of the faces
        o = centre + half * (torch.rand(R, 3, generator=g) * 2 - 1) * 2.5
        d = torch.nn.functional.normalize(centre + half * (torch.rand(R, 3, generator=g) * 2 - 1) * 0.8 - o, dim=-1)
        ri = torch.sort(torch.randint(R, (n,), generator=g)).values.to(torch.int32)
        ts = torch.rand(n, generator=g) * 4.0
        te = ts + torch.rand(n, generator=g) * 0.05
        o[0] = torch.tensor([AABB[0], 0.31, 0.37]); ts[ri == 0] = 0.0; te[ri == 0] = 0.0      # ray 0: a point exactly on a box face
        tm = (ts + te) * 0.5
        xw = (o.double()[ri.long()] + d.double()[ri.long()] * tm.double()[:, None]).float()         # fmaf(d, tm, o), as the kernel
        dfeat = torch.randn(n, 32, generator=g)
        xu = ofield.contract(xw, aabb, ct)
        ur = xu.clone().requires_grad_()
        (g_u,) = torch.autograd.grad((hashgrid.encode(ur, table.double(), spec) * dfeat.double()).sum(), ur)
        x64 = xw.double().requires_grad_()
        (ref,) = torch.autograd.grad(ofield.contract(x64, aabb.double(), ct), x64, g_u.double())    # J_contract^T (float64)
        dist, ulps = face_distance(xu, spec)
        if ct_name == "sphere":
            m = ((xw - aabb[:3]) / (aabb[3:] - aabb[:3]) * 2 - 1).norm(dim=-1)
            assert int((m > 1).sum()) > 50 and int((m < 1).sum()) > 50
        _CACHE[ct_name] = dict(spec=spec, table=table, ct=ct, o=o, d=d, ri=ri, ts=ts, te=te, dfeat=dfeat, ref=ref.double(),
                               safe=dist >= FACE, ulps=ulps, n=n)
    return _CACHE[ct_name]


@pytest.mark.parametrize("ct_name", sorted(SCENES))
def test_bwd_input_scene_form_vs_oracle_and_jvp(amd, ct_name):
    """World-space gradient from the packed sample stream: aabb, tanh and sphere contraction (samples inside and outside the
    unit ball), both layouts, against oracle.field.contract composed with oracle.hashgrid.encode and against the three-launch
    JVP over the same rays.  The seeds are chosen (a CPU property, asserted) so that no compared sample sits within 8 float32
    ulps of a cell face: the GPU's and the CPU's float32 contraction differ by an ulp or two, which must not move a sample
    into the neighbouring cell of the reference.
    Measured (MI355X, aabb / sphere / tanh): (b) vs (a) 1.7e-7 / 1.2e-5 / 7.8e-6, kernel vs (b) 1.5e-7 / 1.2e-7 / 1.9e-7,
    kernel vs (a) rel 2.6e-7 / 1.2e-5 / 7.8e-6, elem 2.8e-5 / 3.5e-4 / 1.8e-3; nothing left out."""
    ops, _ = amd
    c = scene_case(ct_name)
    assert float((~c["safe"]).float().mean()) < 0.01
    assert float(c["ulps"][c["safe"]].min()) >= 8.0, "seed: a compared sample within 8 ulps of a cell face"
    grid, n_params = ops.make_grid_desc(**SCENE_GRID)
    assert n_params == c["spec"].n_params and any(c["spec"].hashed)
    scene = ops.make_scene_desc(AABB, c["ct"])
    n = c["n"]
    td, o, d, ri, ts, te = (dev(c[k]) for k in ("table", "o", "d", "ri", "ts", "te"))
    ref_b = jvp3_scene(ops, grid, td, scene, o, d, ri, ts, te, dev(c["dfeat"])).cpu().double()
    e_ba, scale = b_error(c["ref"], ref_b, c["safe"])
    for layout in (0, 1):
        df = dev(c["dfeat"]) if layout == 0 else dev(to_frag(c["dfeat"]))
        got = ops.hashgrid_bwd_input(grid, td, df, scene=scene, rays=(o, d), samples=(ri, ts, te), n=n, layout=layout)
        check_against_references(got.cpu().double(), c["ref"], ref_b, c["safe"], e_ba, scale, f"{ct_name} layout {layout}",
                                 rel_a=REL_SCENE, elem_a=ELEM_SCENE)


def test_bwd_input_conventions(amd):
    """n = 0 is accepted; dfeat = 0 gives dx == 0 exactly; a grid of fewer levels ignores the levels it does not have"""
    ops, _ = amd
    from oracle import hashgrid
    kw = dict(n_levels=5, log2_hashmap_size=12)
    spec = hashgrid.make_spec(**kw)
    grid, _ = ops.make_grid_desc(**kw)
    table = hashgrid.init_table(spec, 5, 1.0, "mix32")
    td = dev(table)
    x = unit_points(8)[:100].contiguous()
    assert ops.hashgrid_bwd_input(grid, td, torch.zeros(0, 10, device=DEV), x_unit=torch.zeros(0, 3, device=DEV), n=0,
                                  layout=0).shape == (0, 3)
    out = ops.hashgrid_bwd_input(grid, td, torch.zeros(100, 10, device=DEV), x_unit=dev(x), n=100, layout=0)
    assert bool((out == 0).all())
    dfeat = torch.randn(100, 10, generator=torch.Generator().manual_seed(1))
    xr = x.clone().requires_grad_()
    (ref,) = torch.autograd.grad((hashgrid.encode(xr, table.double(), spec) * dfeat.double()).sum(), xr)
    got = ops.hashgrid_bwd_input(grid, td, dev(dfeat), x_unit=dev(x), n=100, layout=0)
    assert rel_err(got.cpu(), ref) < REL_A
    with pytest.raises(NotImplementedError):                                # the fragment layout is 16 levels wide
        ops.hashgrid_bwd_input(grid, td, torch.zeros(4 * 1024, device=DEV), x_unit=dev(x), n=100, layout=1)


# ---------------------------------------------------------------------------------------------- Renderer.density_gradient
GRAD_MARGIN = 4.0       # the gradient's bound = sigma's own bound (1e-4 of the largest value) x this margin: see the test's docstring


def _golden_field(name, tag, full_table_cache):
    import json
    g0 = load_golden(name)
    if tag is None:
        return g0, {}, int(g0["contraction_type"])
    acts = json.loads(str(g0["combos"]))[tag]
    g = {k[len(tag) + 1:]: v for k, v in g0.items() if k.startswith(tag + ".")}
    g.update(aabb=g0["aabb"], table_seed=g0["table_seed"], table_scale=g0["table_scale"])
    return g, acts, 0


@pytest.mark.parametrize("name,tag", [("field_aabb", None), ("field_sphere", None), ("field_tanh", None), ("field_acts", "a")])
def test_density_gradient_vs_oracle_autograd(amd, full_table_cache, name, tag):
    """(sigma, d sigma / d x_world) of Renderer.density_gradient on the golden fields (the three contractions, one alternative
    activation set) at 512 points -- the fixture's own 384, 100 more in the box, 28 outside it (outside the selector only under
    aabb: tanh / sphere contract them into the cube) -- against autograd of
    oracle.field.query_density (float64 parameters, float32 positions).
    Bound: sigma itself is held to the 1e-4 of its largest value that the forward tests use, and the gradient, relative to its
    largest entry, to GRAD_MARGIN = 4 times that: it is the same MLP arithmetic (backward instead of forward) times the
    encoder's Jacobian, whose entries are differences of cell entries times a scale of up to 4096 and cancel.  Measured, the
    gradient's error is 2.7 / 20 / 19 / 1.0 times sigma's own on the four fields and at most 2.6 times sigma's bound.
    Samples compared: under aabb the unit position is two exactly rounded operations, the same bits on both sides, and the
    kernel test's rule holds -- all samples at least 2^-20 of a cell from every face, share left out < 1 %.  Under tanh /
    sphere the contraction runs in float32 on both sides, up to 4 ulps of the unit position and so up to 8 ulps of a level
    position apart, and a sample that close to a face sits in another cell for the oracle than for the kernel: those samples
    are left out.  Their share is a property of the points alone: within 8 ulps of a face on either side, in any of 3
    coordinates and 16 levels, with probability at most 3 x 2 x 8 x ulp(position), and a position uniform in [0, scale_l]
    has an ulp of about 2^-24 scale_l: 48 x 2^-24 x sum_l scale_l (13 300 on this grid) = 3.8 %; asserted < 5 %.
    Outside the box the gradient is exactly zero; the field's parameters, gradient buffers and the occupancy grid are
    bit-identical afterwards.
    Measured (MI355X; aabb / sphere / tanh / field_acts a): sigma 1.2e-7 / 1.3e-5 / 1.1e-5 / 2.6e-7, gradient 3.1e-7 / 2.6e-4 /
    2.0e-4 / 2.7e-7; 0 / 15 / 13 / 0 of 512 points left out."""
    from oracle import field as ofield, hashgrid
    ops, engine = amd
    g, acts, ct = _golden_field(name, tag, full_table_cache)
    spec = hashgrid.make_spec()
    table = full_table_cache(g["table_seed"], g["table_scale"])
    aabb = t(g["aabb"]).float()
    gen = torch.Generator().manual_seed(21)
    lo, hi = aabb[:3], aabb[3:]
    inside = lo + (hi - lo) * torch.rand(100, 3, generator=gen)
    outside = lo + (hi - lo) * (1.0 + 0.5 * torch.rand(28, 3, generator=gen))
    outside[::2] = lo - (hi - lo) * 0.5 * torch.rand(14, 3, generator=gen)
    x = torch.cat([t(g["x"]).float(), inside, outside]).contiguous()
    n = x.shape[0]
    cfg = engine.RenderCfg(aabb=tuple(float(v) for v in aabb), contraction_type=ct, occ_res=(8, 8, 8),
                           **({f"{k}_activation": v for k, v in acts.items()} if acts else {}))
    fld = engine.NGPField(DEV)
    p = field_params_from(g, table)
    fld.load(p)
    r = engine.Renderer(fld, cfg)
    fld.grad_all.normal_(generator=torch.Generator(device=DEV).manual_seed(1))
    r.occs.uniform_(); r.binary.fill_(1)
    before = [b.clone() for b in (fld.flat, fld.grad_all, r.occs, r.binary)]
    sigma, grad = r.density_gradient(dev(x))
    torch.cuda.synchronize()
    for b0, b1 in zip(before, (fld.flat, fld.grad_all, r.occs, r.binary)):
        assert torch.equal(b0, b1), "density_gradient changed the field's state"
    xr = x.clone().requires_grad_()
    p64 = {k: v.double() for k, v in p.items()}
    sig_o = ofield.query_density(xr, p64, spec, aabb, ct, acts=acts or None)[:, 0]
    (grad_o,) = torch.autograd.grad(sig_o.sum(), xr)
    xu = ofield.contract(x, aabb, ct)
    sel = ofield.selector(xu)
    assert int((~sel).sum()) >= (28 if ct == 0 else 0)          # tanh / sphere map every world point into the cube
    assert bool((grad.cpu()[~sel] == 0).all()) and bool((sigma.cpu()[~sel] == 0).all())
    dist, ulps = face_distance(xu, spec)
    safe = ((dist >= FACE) if ct == 0 else (ulps >= 8.0)) | ~sel
    e_sig = rel_err(sigma.cpu(), sig_o)
    e_grad = rel_err(grad.cpu()[safe], grad_o[safe])
    print(f"{name} {tag}: sigma {e_sig:.2e}  gradient {e_grad:.2e} (ratio {e_grad / max(e_sig, 1e-30):.2f})  "
          f"left out {int((~safe).sum())} of {n}; max |grad| {float(grad_o.abs().max()):.3g}")
    assert float((~safe).float().mean()) < (0.01 if ct == 0 else 0.05)
    assert e_sig < 1e-4
    assert e_grad < GRAD_MARGIN * 1e-4


def test_density_gradient_weight_norm_uses_effective_parameters(amd, full_table_cache):
    """a weight-normalised field answers with W = g v / |v|: the same gradient as the plain field holding W"""
    ops, engine = amd
    g = load_golden("field_aabb")
    table = full_table_cache(g["table_seed"], g["table_scale"])
    p = field_params_from(g, table)
    cfg = engine.RenderCfg(aabb=tuple(float(v) for v in g["aabb"]), occ_res=(8, 8, 8))
    plain, wn = engine.NGPField(DEV), engine.NGPField(DEV, weight_norm=(True, True))
    plain.load(p); wn.load(p)
    x = dev(t(g["x"]).float())
    s0, g0 = engine.Renderer(plain, cfg).density_gradient(x)
    s1, g1 = engine.Renderer(wn, cfg).density_gradient(x)
    assert rel_err(s1, s0) < 1e-5 and rel_err(g1, g0) < 1e-5


# ---------------------------------------------------------------------------------------------- render_normal_image
@pytest.fixture(scope="module")
def small_scene(amd):
    """a small random field (table of order 0.3: a dense, bumpy fog), occupancy grid fully on, one camera looking at the box"""
    from oracle import field as ofield, hashgrid
    ops, engine = amd
    spec = hashgrid.make_spec()
    p = ofield.init_params(spec, 1, seed=3, table_kind="uniform", table_scale=0.3)
    fld = engine.NGPField(DEV)
    fld.load(p)
    cfg = engine.RenderCfg(aabb=(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), occ_res=(16, 16, 16), render_step_size=0.05)
    r = engine.Renderer(fld, cfg)
    r.binary.fill_(1)
    H, W = 12, 16
    K = torch.tensor([[20.0, 0.0, W / 2], [0.0, 20.0, H / 2], [0.0, 0.0, 1.0]])
    Kinv = dev(torch.linalg.inv(K))
    a = 0.3
    rot = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])   # camera axes = columns
    pos = torch.tensor([-3.0 * math.sin(a), 0.1, -3.0 * math.cos(a)])                                         # looks along +z_cam at the box
    return types.SimpleNamespace(r=r, fld=fld, Kinv=Kinv, rot=dev(rot), pos=dev(pos), H=H, W=W)


def test_render_normal_image_vs_opwise_recomputation(amd, small_scene):
    """16 x 12 normal map = the op-wise recomputation on the same rays and samples (per-sample gradients through reference
    (b), a torch loop for sum_i w_i n_i) within the composite test's tolerance (test_gpu_parity.py: rel_err < 1e-5);
    |N| <= opacity + 1e-5; camera frame = R^T world frame; a ray that looks away gives exactly zero."""
    from robust_e_nerf_amd import evaluation
    ops, engine = amd
    s = small_scene
    r, f = s.r, s.fld
    px = evaluation.pixel_grid(s.H, s.W, DEV).reshape(-1, 2)
    nr = px.shape[0]
    pos, rot = s.pos.expand(nr, 3).contiguous(), s.rot.expand(nr, 3, 3).contiguous()
    world, opac, cam = evaluation.render_normals(r, s.Kinv, px, pos, rot)
    img, opac_img = evaluation.render_normal_image(r, s.Kinv, s.pos, s.rot, s.H, s.W)
    assert img.shape == (3, s.H, s.W) and opac_img.shape == (s.H, s.W)
    assert torch.equal(img.permute(1, 2, 0).reshape(-1, 3), cam) and torch.equal(opac_img.reshape(-1), opac)
    assert float(opac.max()) > 0.05 and float(world.abs().max()) > 0            # the scene is not empty
    assert bool((world.norm(dim=-1) <= opac + 1e-5).all())
    assert rel_err(cam, torch.einsum("nij,ni->nj", rot, world)) < 1e-6
    # op-wise: same rays, same samples
    o, d = ops.raygen(s.Kinv, px.contiguous(), pos, rot)
    pk = r.sample(o, d, None, False)
    smp = (pk.ray_indices, pk.t_starts, pk.t_ends)
    feat = ops.hashgrid_fwd(f.grid, f.table, scene=r.scene, rays=(o, d), samples=smp, n=pk.n, layout=1)
    _, sigma, base = ops.mlp_fwd(f.mlp, 1, feat, r.scene, rays=(o, d), samples=smp, n=pk.n, density_only=True, save_base=True)
    zero = torch.zeros(pk.n, 1, device=DEV)
    dfeat = ops.mlp_bwd(f.mlp, 1, feat, base, r.scene, rays=(o, d), samples=smp, n=pk.n, rgb=zero, d_rgb=zero,
                        d_sigma=torch.ones(pk.n, device=DEV), grad_mlp_params=torch.zeros(f.n_mlp, device=DEV),
                        workspace=torch.empty(ops.mlp_bwd_workspace_floats(1), device=DEV))
    from robust_e_nerf_amd import tcnn_api
    grad_b = jvp3_scene(ops, f.grid, f.table, r.scene, o, d, *smp, tcnn_api._to_rows(dfeat, pk.n))
    nrm = (-grad_b / grad_b.norm(dim=-1, keepdim=True).clamp_min(1e-12)).cpu().double()
    ts, te, sg = pk.t_starts.cpu().double(), pk.t_ends.cpu().double(), sigma.cpu().double()
    offs, cnts = pk.offsets.cpu().tolist(), pk.counts.cpu().tolist()
    ref = torch.zeros(nr, 3, dtype=torch.float64)
    ref_o = torch.zeros(nr, dtype=torch.float64)
    for ray in range(nr):
        T = 1.0
        for i in range(offs[ray], offs[ray] + cnts[ray]):
            a = 1.0 - math.exp(-float(sg[i]) * float(te[i] - ts[i]))
            ref[ray] += T * a * nrm[i]
            ref_o[ray] += T * a
            T *= 1.0 - a
    e_n, e_o = rel_err(world.cpu(), ref), rel_err(opac.cpu(), ref_o)
    print(f"normal image vs op-wise: normals {e_n:.2e} opacity {e_o:.2e} ({pk.n} samples, largest |N| {float(ref.abs().max()):.3f})")
    assert e_n < 1e-5 and e_o < 1e-5
    # a ray that looks away from the box
    back = s.rot.clone()
    back[:, 2] = -back[:, 2]; back[:, 0] = -back[:, 0]
    w2, o2, c2 = evaluation.render_normals(r, s.Kinv, px[:3].contiguous(), pos[:3].contiguous(), back.expand(3, 3, 3).contiguous())
    assert bool((w2 == 0).all()) and bool((o2 == 0).all()) and bool((c2 == 0).all())


def test_render_normal_image_chunks_and_rows(amd, small_scene):
    """independent of `chunk` (one chunk vs chunks of 50 rays, bit for bit: a ray's samples do not depend on its neighbours);
    a rows= band equals the same rows of the full image"""
    from robust_e_nerf_amd import evaluation
    s = small_scene
    full, fo = evaluation.render_normal_image(s.r, s.Kinv, s.pos, s.rot, s.H, s.W)
    ch, co = evaluation.render_normal_image(s.r, s.Kinv, s.pos, s.rot, s.H, s.W, chunk=50)
    assert torch.equal(full, ch) and torch.equal(fo, co)
    band, bo = evaluation.render_normal_image(s.r, s.Kinv, s.pos, s.rot, s.H, s.W, rows=(3, 8))
    assert torch.equal(band, full[:, 3:8]) and torch.equal(bo, fo[3:8])


def test_normals_refuse_arch_mlp(amd):
    from robust_e_nerf_amd import evaluation, vanilla
    r = vanilla.VanillaRenderer.__new__(vanilla.VanillaRenderer)            # no field needed: the refusal comes first
    r.field = object()
    with pytest.raises(NotImplementedError, match="normals: arch ngp only"):
        r.density_gradient(torch.zeros(4, 3, device=DEV))
    with pytest.raises(NotImplementedError, match="normals: arch ngp only"):
        evaluation.render_normal_image(r, torch.eye(3, device=DEV), torch.zeros(3, device=DEV), torch.eye(3, device=DEV), 4, 4)

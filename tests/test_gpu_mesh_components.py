"""Lattice components on the GPU (csrc/ren_mesh_components.hip, mesh.components / mesh.clean) against the numpy restatement
tests/mesh_components_reference.py: label, size and border with `torch.equal`, every case.  The outputs are functions of the
lattice alone, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import mesh_components_reference as cref
from test_gpu_mesh import golden_renderer  # noqa: F401  (the tiny arch-ngp renderer, a module-scoped fixture)
from test_mesh_cpu import read_ply

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LO, HI = (-1.5, 0.25, 2.0), (2.5, 1.75, 3.5)


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import _lib, mesh, ops
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops, mesh


_REF = {}


def reference(key, sigma, level, outside):
    """the restatement of one case, computed once and handed out read-only"""
    if key not in _REF:
        out = cref.components(sigma, level, outside)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(ops, sigma, level, outside, want, tag):
    label, size, border = ops.mesh_components(dev(sigma.astype(np.float32)), level, outside)
    n = sigma.size
    assert label.shape == sigma.shape and label.dtype == torch.int32
    assert size.shape == (n,) and size.dtype == torch.int32 and border.shape == (n,) and border.dtype == torch.uint8
    w_label, w_size, w_border = (torch.from_numpy(np.array(a)) for a in want)
    assert torch.equal(label.cpu(), w_label), (tag, "label")
    assert torch.equal(size.cpu(), w_size), (tag, "size")
    assert torch.equal(border.cpu(), w_border), (tag, "border")
    return label, size, border


# ---------------------------------------------------------------------------------------------------- random lattices
@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("share", [0.15, 0.30])
@pytest.mark.parametrize("res", [(13, 11, 9), (33, 17, 9)])
def test_random_lattices(amd, res, share, outside):
    ops, _ = amd
    sigma, level = cref.random_lattice(res, share)
    want = reference(("random", res, share, outside), sigma, level, outside)
    if not outside:                                   # from the restatement: the case is not vacuous
        w_label, w_size, _ = want
        roots = np.flatnonzero(w_size)
        flat = w_label.reshape(-1)
        spanning = sum(1 for r in roots if len(set((np.flatnonzero(flat == r) // 256).tolist())) > 1)
        print(res, share, len(roots), int((w_size[roots] > 1).sum()), spanning, int(w_size.max()))
        if share == 0.15:
            assert len(roots) >= 30 and (w_size[roots] > 1).sum() >= 10 and spanning >= 10
        else:
            assert w_size.max() > 300
    check(ops, sigma, level, outside, want, f"random {res} {share} {outside}")


# ---------------------------------------------------------------------------------------------------- chains
def _chain(name):
    if name.startswith("serpentine"):                 # one point wide through the middle plane of 17 x 17 x 3
        inside = np.zeros((17, 17, 3), dtype=bool)
        for i in range(0, 17, 2):
            inside[i, :, 1] = True
            if i + 1 < 17:
                inside[i + 1, 16 if i % 4 == 0 else 0, 1] = True
    elif name.startswith("staircase"):                # steps +x, +y, +z in turn from (0, 0, 0) to (23, 23, 23)
        inside = np.zeros((24, 24, 24), dtype=bool)
        p = [0, 0, 0]
        inside[tuple(p)] = True
        for step in range(69):
            p[step % 3] += 1
            inside[tuple(p)] = True
    else:                                             # the body diagonal alone: every link is the direction (1, 1, 1)
        inside = np.zeros((24, 24, 24), dtype=bool)
        for t in range(2, 21):
            inside[t, t, t] = True
    if name.endswith("mirrored"):
        inside = inside[::-1, ::-1, ::-1]
    return np.where(inside, np.float32(1), np.float32(-1)).astype(np.float32)


@pytest.mark.parametrize("name", ["serpentine", "serpentine_mirrored", "staircase", "staircase_mirrored", "diagonal"])
def test_chains_are_one_component(amd, name):
    ops, _ = amd
    sigma = _chain(name)
    want = reference(("chain", name), sigma, 0.0, False)
    first = int(np.flatnonzero(sigma.reshape(-1) > 0)[0])
    assert np.flatnonzero(want[1]).tolist() == [first] and want[1][first] == (sigma > 0).sum()   # the restatement: one component
    label, size, _ = check(ops, sigma, 0.0, False, want, name)
    assert int(label.max()) == first and int(size[first]) == int((sigma > 0).sum())


# ---------------------------------------------------------------------------------------------------- contention
def test_all_inside_is_one_component(amd):
    ops, _ = amd
    sigma = np.ones((33, 17, 9), dtype=np.float32)
    label, size, border = check(ops, sigma, 0.5, False, reference("all_inside", sigma, 0.5, False), "all inside")
    assert int(size[0]) == sigma.size and int(size.sum()) == sigma.size and int(border.sum()) == 1
    check(ops, sigma, 0.5, True, reference("all_inside_out", sigma, 0.5, True), "all inside, outside")


def test_all_inside_over_1024_workgroups(amd):
    """64^3: 1 024 workgroups on every XCD unite into the root 0 (the expectation needs no restatement)"""
    ops, _ = amd
    n = 64 ** 3
    label, size, border = ops.mesh_components(torch.full((64, 64, 64), 2.0, device=DEV), 1.0)
    assert int(label.abs().max()) == 0
    assert int(size[0]) == n and int(size.count_nonzero()) == 1
    assert int(border[0]) == 1 and int(border.count_nonzero()) == 1


def test_all_outside_is_empty(amd):
    ops, _ = amd
    sigma = np.zeros((33, 17, 9), dtype=np.float32)
    label, size, border = check(ops, sigma, 0.5, False, reference("all_outside", sigma, 0.5, False), "all outside")
    assert bool((label == -1).all()) and not bool(size.any()) and not bool(border.any())


# ---------------------------------------------------------------------------------------------------- extents, special values
@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("res", [(2, 2, 2), (2, 33, 2), (5, 3, 70)])
def test_extents(amd, res, outside):
    ops, _ = amd
    sigma, level = cref.random_lattice(res, 0.4, seed=11)
    check(ops, sigma, level, outside, reference(("extent", res, outside), sigma, level, outside), f"extent {res}")


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("case", ["nan", "inf", "neg_inf", "level_in_field"])
def test_special_values(amd, case, outside):
    ops, _ = amd
    sigma = np.random.default_rng(5).uniform(-1.0, 1.0, (5, 4, 3)).astype(np.float32)
    level = 0.0
    special = [(2, 1, 1), (0, 0, 0), (4, 3, 2)]
    value = {"nan": np.nan, "inf": np.inf, "neg_inf": -np.inf, "level_in_field": float(sigma[3, 1, 1])}[case]
    if case == "level_in_field":
        level = value
    for p in special:
        sigma[p] = value
    want = reference(("special", case, outside), sigma, level, outside)
    label, _, _ = check(ops, sigma, level, outside, want, case)
    member = {"nan": outside, "inf": not outside, "neg_inf": outside, "level_in_field": not outside}[case]   # as in "mesh"
    for p in special:
        assert (int(label[p]) >= 0) == member, (case, p)


# ---------------------------------------------------------------------------------------------------- apply
def test_apply_keeps_bit_patterns_and_may_alias(amd):
    ops, _ = amd
    sigma_np, level = cref.random_lattice((13, 11, 9), 0.15)
    sigma_np = sigma_np.copy()
    bits = sigma_np.view(np.int32)
    bits[3, 4, 5] = 0x7FC12345                        # NaNs with payloads, one of them negative, and a negative zero
    bits[0, 0, 0] = -0x3FEDCB
    bits[12, 10, 8] = -0x80000000
    sigma = dev(sigma_np)
    label, size, _ = ops.mesh_components(sigma, level)
    n = sigma.numel()
    none = torch.zeros(n, device=DEV, dtype=torch.uint8)
    out = ops.mesh_component_apply(sigma, label, none, -np.inf)
    assert out.data_ptr() != sigma.data_ptr() and torch.equal(out.view(torch.int32), sigma.view(torch.int32))
    roots = torch.nonzero(size).reshape(-1)
    marked = roots[::2]
    drop = none.clone()
    drop[marked] = 1
    out = ops.mesh_component_apply(sigma, label, drop, -np.inf)
    hit = torch.isin(label, marked.to(torch.int32))
    assert int(hit.sum()) == int(size[marked].sum()) > 0
    assert bool((out[hit] == -np.inf).all())
    assert torch.equal(out.view(torch.int32)[~hit], sigma.view(torch.int32)[~hit])
    drop[torch.nonzero(label.reshape(-1) < 0).reshape(-1)[:5]] = 1                # marks at indices that are no roots: nothing
    assert torch.equal(ops.mesh_component_apply(sigma, label, drop, -np.inf).view(torch.int32), out.view(torch.int32))
    alias = sigma.clone()
    back = ops.mesh_component_apply(alias, label, drop, -np.inf, out=alias)
    assert back.data_ptr() == alias.data_ptr() and torch.equal(alias.view(torch.int32), out.view(torch.int32))
    flat = ops.mesh_component_apply(sigma.reshape(-1), label.reshape(-1), drop, 7.5)                  # any shape
    assert torch.equal(flat.reshape(sigma.shape)[hit], torch.full_like(out[hit], 7.5))


# ---------------------------------------------------------------------------------------------------- clean + extract
def two_balls_and_a_floater():
    sigma = np.maximum(cref.ball((24,) * 3, (7.2, 7.9, 8.1), 4.6), cref.ball((24,) * 3, (16.1, 15.8, 15.2), 3.3))
    sigma[20, 3, 4] = 0.5
    return sigma


def shell(floater):
    d = cref.ball((16,) * 3, (7.3, 7.6, 7.4), 0.0)                                # -distance
    sigma = np.minimum(d + np.float32(6.2), -d - np.float32(3.1))                 # inside between the radii 3.1 and 6.2
    if floater:
        sigma[7, 8, 7] = 0.5
    return sigma


def clean_and_extract(mesh, sigma_np, want_stats=None, **rule):
    """mesh.clean on the device against the restatement's cleaned lattice, then both through the same mesh.extract"""
    want, stats = cref.clean(sigma_np, 0.0, **rule)
    sigma = dev(sigma_np)
    before = sigma.clone()
    got, got_stats = mesh.clean(sigma, 0.0, **rule)
    assert torch.equal(sigma, before)                                             # the input is never written
    assert got_stats == stats and (want_stats is None or {k: stats[k] for k in want_stats} == want_stats)
    assert torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(want).view(torch.int32))
    verts, faces = mesh.extract(got, 0.0, LO, HI)
    v_ref, f_ref = mesh.extract(dev(want), 0.0, LO, HI)
    assert torch.equal(verts, v_ref) and torch.equal(faces, f_ref)
    assert bool(torch.isfinite(verts).all())
    return got, verts, faces


@pytest.mark.parametrize("rule", [dict(min_points=2), dict(largest=1)], ids=["min_points", "largest"])
def test_clean_drops_floaters(amd, rule):
    _, mesh = amd
    sigma_np = two_balls_and_a_floater()
    kept = 2 if "min_points" in rule else 1
    got, verts, faces = clean_and_extract(mesh, sigma_np, dict(components=3, kept=kept, cavities=0), **rule)
    v_all, f_all = mesh.extract(dev(sigma_np), 0.0, LO, HI)
    assert 0 < faces.shape[0] < f_all.shape[0]
    rows = {r.tobytes() for r in v_all.cpu().numpy()}
    assert all(r.tobytes() in rows for r in verts.cpu().numpy())                  # a subset, bit for bit
    assert float(got[20, 3, 4]) == -np.inf


def test_clean_without_anything_to_do_returns_its_input(amd):
    _, mesh = amd
    sigma = dev(two_balls_and_a_floater())
    for rule in (dict(), dict(largest=3), dict(fill_cavities=True)):
        got, stats = mesh.clean(sigma, 0.0, **rule)
        assert got is sigma and stats == dict(components=3, kept=3, dropped_points=0, cavities=0, filled_points=0)


def test_clean_fills_a_hollow_shell(amd):
    _, mesh = amd
    sigma_np = shell(floater=False)
    _, _, faces = clean_and_extract(mesh, sigma_np, dict(components=1, kept=1, dropped_points=0, cavities=1), fill_cavities=True)
    _, f_shell = mesh.extract(dev(sigma_np), 0.0, LO, HI)
    _, f_outer = mesh.extract(dev(cref.ball((16,) * 3, (7.3, 7.6, 7.4), 6.2)), 0.0, LO, HI)       # the solid ball: the outer surface alone
    assert faces.shape[0] == f_outer.shape[0] < f_shell.shape[0]
    assert torch.equal(faces, f_outer)


def test_floater_in_a_cavity_is_dropped_and_then_filled_over(amd):
    """the order of the two steps: filled after the drop the floater's point is part of the cavity; the other way round it
    would stay a -inf hole inside the filled solid"""
    _, mesh = amd
    sigma_np = shell(floater=True)
    got, _, faces = clean_and_extract(mesh, sigma_np, dict(components=2, kept=1, dropped_points=1, cavities=1), min_points=2,
                                      fill_cavities=True)
    assert float(got[7, 8, 7]) == np.inf
    _, f_outer = mesh.extract(dev(cref.ball((16,) * 3, (7.3, 7.6, 7.4), 6.2)), 0.0, LO, HI)
    assert torch.equal(faces, f_outer)
    only_fill, stats = mesh.clean(dev(sigma_np), 0.0, fill_cavities=True)         # without the drop the floater stays inside
    assert stats["cavities"] == 1 and float(only_fill[7, 8, 7]) == 0.5


def test_mesh_components_lists_the_roots(amd):
    _, mesh = amd
    sigma_np, level = cref.random_lattice((33, 17, 9), 0.15)
    w_label, w_size, w_border = reference(("random", (33, 17, 9), 0.15, False), sigma_np, level, False)
    label, roots, sizes, border = mesh.components(dev(sigma_np), level)
    w_roots = np.flatnonzero(w_size)
    assert roots.dtype == torch.int64 and roots.cpu().tolist() == w_roots.tolist()
    assert sizes.cpu().tolist() == w_size[w_roots].tolist() and border.cpu().tolist() == w_border[w_roots].tolist()
    assert torch.equal(label.cpu(), torch.from_numpy(np.array(w_label)))


# ---------------------------------------------------------------------------------------------------- repeatability
def test_two_runs_are_bit_identical(amd):
    ops, mesh = amd
    sigma_np, level = cref.random_lattice((33, 17, 9), 0.30)
    sigma = dev(sigma_np)
    for outside in (False, True):
        a, b = ops.mesh_components(sigma, level, outside), ops.mesh_components(sigma, level, outside)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    label, size, _ = a
    drop = (size > 0).to(torch.uint8)
    x, y = ops.mesh_component_apply(sigma, label, drop, np.inf), ops.mesh_component_apply(sigma, label, drop, np.inf)
    assert torch.equal(x, y)
    (c0, s0), (c1, s1) = mesh.clean(sigma, level, largest=2, fill_cavities=True), mesh.clean(sigma, level, largest=2, fill_cavities=True)
    assert torch.equal(c0, c1) and s0 == s1


# ---------------------------------------------------------------------------------------------------- export
def vanilla_renderer():
    from robust_e_nerf_amd import config, engine, vanilla
    fld = vanilla.VanillaField(DEV, 1)
    config.init_field(fld, "mlp", 1, torch.Generator().manual_seed(0))
    return vanilla.VanillaRenderer(fld, engine.RenderCfg(aabb=(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0))), (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


@pytest.mark.parametrize("arch", ["ngp", "mlp"])
def test_export_with_and_without_cleaning(amd, arch, request, tmp_path, monkeypatch):
    ops, mesh = amd
    r, aabb = request.getfixturevalue("golden_renderer") if arch == "ngp" else vanilla_renderer()
    res, normals = (24, True) if arch == "ngp" else (12, False)
    lo, hi = aabb[:3], aabb[3:]
    sigma = mesh.sample_density(r, lo, hi, res)
    level = float(sigma.median())
    # the defaults: today's file, byte for byte, and no labelling at all
    verts, faces = mesh.extract(sigma, level, lo, hi)
    by_hand, default = str(tmp_path / "by_hand.ply"), str(tmp_path / "default.ply")
    mesh.write_ply(by_hand, verts, faces, mesh.vertex_normals(r, verts) if normals else None)

    def refuse(*a, **k):
        raise AssertionError("mesh.export labelled components without being asked to")
    with monkeypatch.context() as m:
        m.setattr(ops, "mesh_components", refuse)
        stats = mesh.export(r, default, res, level, normals=normals)
    assert stats == dict(verts=verts.shape[0], faces=faces.shape[0], resolution=(res,) * 3, normals=normals)
    assert open(default, "rb").read() == open(by_hand, "rb").read()
    # largest = 1
    _, roots, sizes, _ = mesh.components(sigma, level)
    print(arch, "components", roots.numel(), "sizes", sorted(sizes.cpu().tolist())[-3:])
    if arch == "ngp":
        assert roots.numel() > 1, "the field has one component only: the case shows nothing"
    cleaned = str(tmp_path / "largest.ply")
    stats1 = mesh.export(r, cleaned, res, level, normals=normals, largest=1)
    v1, f1, n1 = read_ply(cleaned)
    assert (stats1["verts"], stats1["faces"], stats1["resolution"], stats1["normals"]) == (len(v1), len(f1), (res,) * 3, normals)
    assert (n1 is not None) == normals
    assert stats1["components"] == roots.numel() and stats1["kept"] == 1
    assert stats1["dropped_points"] == int(sizes.sum()) - int(sizes.max()) and stats1["cavities"] == stats1["filled_points"] == 0
    assert 0 < len(f1) <= faces.shape[0] and (len(f1) < faces.shape[0]) == (roots.numel() > 1)
    assert f1.min() >= 0 and f1.max() == len(v1) - 1
    rows = {row.tobytes() for row in verts.cpu().numpy()}
    assert all(row.tobytes() in rows for row in v1)

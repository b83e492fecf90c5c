"""CPU: the numpy restatement of the lattice components (tests/mesh_components_reference.py) against scipy and against the
definition's corner cases, before the GPU tests hold the kernels to it; mesh.clean's rules; argument validation; the command
line; and the reason mesh.extract needs no change: the vertices of a cleaned lattice are a subset of the original's."""
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import mesh_components_reference as cref
import mesh_reference as ref
from conftest import REPO

RANDOM_CASES = [((13, 11, 9), 0.15), ((13, 11, 9), 0.30), ((33, 17, 9), 0.15), ((33, 17, 9), 0.30)]


def relabel_to_smallest_index(lab):
    """scipy's labels 1 .. C -> the smallest linear index of each component, 0 -> -1"""
    flat = lab.reshape(-1)
    out = np.full(flat.shape, -1, dtype=np.int32)
    for c in range(1, int(flat.max()) + 1):
        idx = np.flatnonzero(flat == c)
        out[idx] = idx[0]
    return out.reshape(lab.shape)


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("res,share", RANDOM_CASES)
def test_restatement_agrees_with_scipy(res, share, outside):
    ndimage = pytest.importorskip("scipy").ndimage
    structure = np.zeros((3, 3, 3), dtype=bool)
    structure[1, 1, 1] = True
    for d in cref.NEIGHBOURS:
        structure[1 + d[0], 1 + d[1], 1 + d[2]] = True
    assert structure.sum() == 15
    sigma, level = cref.random_lattice(res, share)
    label, size, border = cref.components(sigma, level, outside)
    lab, count = ndimage.label(cref.selected(sigma, level, outside), structure=structure)
    assert np.array_equal(label, relabel_to_smallest_index(lab))
    roots = np.flatnonzero(size)
    assert len(roots) == count and np.array_equal(roots, np.unique(label[label >= 0]))
    assert np.array_equal(size[roots], np.bincount(label[label >= 0], minlength=size.size)[roots])
    i, j, k = np.meshgrid(*(np.arange(n) for n in res), indexing="ij")
    face = ((i == 0) | (i == res[0] - 1) | (j == 0) | (j == res[1] - 1) | (k == 0) | (k == res[2] - 1)) & (label >= 0)
    want = np.zeros(size.size, dtype=np.uint8)
    want[np.unique(label[face])] = 1
    assert np.array_equal(border, want)


def test_the_seven_directions_join_and_the_other_six_do_not():
    """each of the 13 direction pairs of the 26-neighbourhood on a lattice with two inside points"""
    joined = 0
    for d in itertools.product((-1, 0, 1), repeat=3):
        if d <= (0, 0, 0):                                                        # one of each pair +-d
            continue
        sigma = np.zeros((3, 3, 3), dtype=np.float32)
        a = tuple(1 if c < 0 else 0 for c in d)
        b = tuple(p + c for p, c in zip(a, d))
        sigma[a] = sigma[b] = 1.0
        label, size, _ = cref.components(sigma, 0.5)
        n_components = int((size > 0).sum())
        is_edge = d in cref.DIRS or tuple(-c for c in d) in cref.DIRS
        assert n_components == (1 if is_edge else 2), d
        assert int(size.sum()) == 2 and (label >= 0).sum() == 2
        joined += is_edge
    assert joined == 7
    # the same neighbourhood for the complement
    sigma = np.ones((2, 2, 2), dtype=np.float32)
    sigma[0, 1, 0] = sigma[1, 0, 0] = 0.0                                         # (1, -1, 0): no edge
    assert int((cref.components(sigma, 0.5, outside=True)[1] > 0).sum()) == 2
    sigma = np.ones((2, 2, 2), dtype=np.float32)
    sigma[0, 0, 0] = sigma[1, 1, 0] = 0.0                                         # (1, 1, 0): an edge
    assert int((cref.components(sigma, 0.5, outside=True)[1] > 0).sum()) == 1


def test_special_values_in_the_restatement():
    sigma = np.full((2, 2, 2), -1.0, dtype=np.float32)
    sigma[0, 0, 0], sigma[0, 0, 1], sigma[1, 1, 1], sigma[1, 0, 1] = np.nan, np.inf, -np.inf, 0.25
    label, size, border = cref.components(sigma, 0.25)
    assert label.reshape(-1).tolist() == [-1, 1, -1, -1, -1, 1, -1, -1] and size[1] == 2 and border[1] == 1
    label, size, _ = cref.components(sigma, 0.25, outside=True)
    assert label.reshape(-1).tolist() == [0, -1, 0, 0, 0, -1, 0, 0] and size[0] == 6            # NaN is a member of the complement


@pytest.mark.parametrize("use", ["restatement", "package"])
def test_clean_ranking_rule(use):
    """sizes in ascending order of the roots; a tie goes to the smaller root"""
    from robust_e_nerf_amd import mesh
    if use == "package":
        kept = lambda s, **kw: mesh.kept_components(torch.tensor(s, dtype=torch.int32), **kw).tolist()
    else:
        kept = lambda s, **kw: cref.kept(s, **kw).tolist()
    sizes = [3, 7, 1, 7, 2, 3]
    assert kept(sizes) == [True] * 6
    assert kept(sizes, min_points=3) == [True, True, False, True, False, True]
    assert kept(sizes, largest=1) == [False, True, False, False, False, False]                   # 7 twice: the smaller root
    assert kept(sizes, largest=2) == [False, True, False, True, False, False]
    assert kept(sizes, largest=3) == [True, True, False, True, False, False]                     # 3 twice: the smaller root
    assert kept(sizes, largest=4, min_points=4) == [False, True, False, True, False, False]
    assert kept(sizes, largest=99) == [True] * 6
    assert kept([]) == [] and kept([], largest=1) == []
    if use == "package":
        for bad in (dict(min_points=0), dict(largest=0), dict(min_points=-3), dict(largest=1.5)):
            with pytest.raises(ValueError):
                kept(sizes, **bad)


def _two_balls_and_a_floater():
    sigma = np.maximum(cref.ball((24,) * 3, (7.2, 7.9, 8.1), 4.6), cref.ball((24,) * 3, (16.1, 15.8, 15.2), 3.3))
    sigma[20, 3, 4] = 0.5
    return sigma


def test_clean_restatement_on_two_balls_and_a_floater():
    sigma = _two_balls_and_a_floater()
    _, size, _ = cref.components(sigma, 0.0)
    sizes = size[size > 0].tolist()
    assert len(sizes) == 3 and sorted(sizes)[0] == 1 and len(set(sizes)) == 3
    out, stats = cref.clean(sigma, 0.0, min_points=2)
    assert stats == dict(components=3, kept=2, dropped_points=1, cavities=0, filled_points=0)
    assert out[20, 3, 4] == -np.inf and (out != sigma).sum() == 1
    out, stats = cref.clean(sigma, 0.0, largest=1)
    assert stats["kept"] == 1 and stats["dropped_points"] == sum(sizes) - max(sizes)
    assert int((cref.components(out, 0.0)[1] > 0).sum()) == 1
    same, stats = cref.clean(sigma, 0.0)
    assert np.array_equal(same, sigma) and stats["kept"] == 3


def _rows(verts):
    return {row.tobytes() for row in np.ascontiguousarray(verts, dtype=np.float32)}


@pytest.mark.parametrize("case", ["floater", "cavity"])
def test_vertices_of_the_cleaned_lattice_are_a_subset_bit_for_bit(case):
    """the +-inf of a rewritten point is never read: every vertex row of extract(clean(sigma)) occurs among extract(sigma)'s"""
    lo, hi = (-1.5, 0.25, 2.0), (2.5, 1.75, 3.5)
    if case == "floater":
        sigma = np.maximum(cref.ball((12,) * 3, (4.2, 4.9, 5.1), 3.1), cref.ball((12,) * 3, (9.1, 8.8, 8.2), 1.4))
        sigma[1, 10, 1] = 0.5
        cleaned, stats = cref.clean(sigma, 0.0, largest=1)
        assert stats["components"] == 3 and stats["kept"] == 1
    else:
        d = cref.ball((12,) * 3, (5.3, 5.6, 5.4), 0.0)                            # -distance
        sigma = np.minimum(d + np.float32(4.4), -d - np.float32(2.1))             # a shell between the radii 2.1 and 4.4
        sigma[5, 6, 5] = 0.5                                                      # and a floater in its cavity
        cleaned, stats = cref.clean(sigma, 0.0, min_points=2, fill_cavities=True)
        assert stats["components"] == 2 and stats["kept"] == 1 and stats["cavities"] == 1 and stats["filled_points"] > 20
        assert cleaned[5, 6, 5] == np.inf                                         # dropped, then filled over
    before = ref.extract(sigma, 0.0, lo, hi)
    after = ref.extract(cleaned, 0.0, lo, hi)
    assert 0 < len(after[0]) < len(before[0]) and 0 < len(after[1]) < len(before[1])
    assert np.isfinite(after[0]).all()
    assert _rows(after[0]) <= _rows(before[0])
    assert ref.topology(after[0], after[1])["closed"]


# ---------------------------------------------------------------------------------------------------- argument validation
def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    from robust_e_nerf_amd import mesh, ops
    sigma = torch.zeros(3, 3, 3)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_components(sigma, 0.0)
    with pytest.raises(ValueError, match="every extent >= 2"):
        ops.mesh_components(torch.zeros(3, 1, 3), 0.0)
    with pytest.raises(ValueError, match="NaN"):
        ops.mesh_components(sigma, float("nan"))
    with pytest.raises(ValueError, match="2\\^30"):                               # a stride-0 view: no memory behind it
        ops.mesh_components(torch.zeros(1).expand(1025, 1024, 1024), 0.0)
    label, drop = torch.zeros(3, 3, 3, dtype=torch.int32), torch.zeros(27, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CPU tensor"):
        ops.mesh_component_apply(sigma, label, drop, 0.0)
    with pytest.raises(ValueError, match="label must be"):
        ops.mesh_component_apply(sigma, label.reshape(-1), drop, 0.0)
    with pytest.raises(ValueError, match="label must be"):
        ops.mesh_component_apply(sigma, label, drop[:-1], 0.0)
    with pytest.raises(ValueError, match="out must be"):
        ops.mesh_component_apply(sigma, label, drop, 0.0, out=torch.zeros(27))
    with pytest.raises(ValueError, match="NaN"):
        ops.mesh_component_apply(sigma, label, drop, float("nan"))
    for bad in (dict(min_points=0), dict(largest=0)):
        with pytest.raises(ValueError, match=">= 1"):
            mesh.clean(sigma, 0.0, **bad)
        with pytest.raises(ValueError, match=">= 1"):
            mesh.export(None, "x.ply", 4, 0.0, (0, 0, 0), (1, 1, 1), **bad)
    with pytest.raises(ValueError, match="finite"):
        mesh.clean(sigma, float("inf"), min_points=2)
    with pytest.raises(ValueError, match="CPU tensor"):
        mesh.clean(sigma, 0.0, min_points=2)
    with pytest.raises(ValueError, match="CPU tensor"):
        mesh.components(sigma, 0.0)


def test_library_refuses_bad_arguments_before_any_launch():
    """both entry points return REN_ERR_BAD_ARG without a device"""
    import ctypes
    from robust_e_nerf_amd import _lib, build
    build.build()
    lib = _lib.load()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)        # aligned / misaligned non-null addresses: nothing is dereferenced
    bad = _lib.REN_ERR_BAD_ARG
    comp, apply = lib.ren_mesh_components, lib.ren_mesh_component_apply
    for ext in ((1, 2, 2), (2, 1, 2), (2, 2, 1), (0, 4, 4), (-2, 4, 4)):
        assert comp(one, *ext, 0.0, 0, one, one, one, None) == bad
    assert comp(one, 1025, 1024, 1024, 0.0, 0, one, one, one, None) == bad
    assert comp(one, 2, 2, 2, float("nan"), 0, one, one, one, None) == bad
    for outside in (2, -1):
        assert comp(one, 2, 2, 2, 0.0, outside, one, one, one, None) == bad
    for null in range(4):
        ptrs = [one] * 4
        ptrs[null] = None
        assert comp(ptrs[0], 2, 2, 2, 0.0, 0, ptrs[1], ptrs[2], ptrs[3], None) == bad
    for off in range(3):                                          # sigma, label, size: 4-byte elements; border: bytes
        ptrs = [one] * 3
        ptrs[off] = odd
        assert comp(ptrs[0], 2, 2, 2, 0.0, 0, ptrs[1], ptrs[2], one, None) == bad
    assert apply(one, one, one, -1, 0.0, one, None) == bad
    assert apply(one, one, one, 2 ** 30 + 1, 0.0, one, None) == bad
    assert apply(one, one, one, 8, float("nan"), one, None) == bad
    for null in range(4):
        ptrs = [one] * 4
        ptrs[null] = None
        assert apply(ptrs[0], ptrs[1], ptrs[2], 8, 0.0, ptrs[3], None) == bad
    assert apply(odd, one, one, 8, 0.0, one, None) == bad
    assert apply(one, odd, one, 8, 0.0, one, None) == bad
    assert apply(one, one, one, 8, 0.0, odd, None) == bad
    assert apply(one, one, odd, 0, float("-inf"), one, None) == _lib.REN_OK                      # no points: nothing is launched


def test_header_and_ctypes_table_name_the_new_entry_points():
    from robust_e_nerf_amd import _lib, build
    hdr = open(os.path.join(REPO, "include", "ren_amd.h")).read()
    for name in ("ren_mesh_components", "ren_mesh_component_apply"):
        assert name in _lib.SIGNATURES and f"int {name}(" in hdr
    assert hdr.index("---- mesh components") > hdr.index("---- mesh (csrc/ren_mesh.hip)")
    assert "ren_mesh_components.hip" in build.SOURCES and build.SOURCES.index("ren_mesh.hip") < build.SOURCES.index("ren_mesh_components.hip")


# ---------------------------------------------------------------------------------------------------- command line
def test_export_mesh_parses_the_cleaning_flags():
    spec = importlib.util.spec_from_file_location("export_mesh", os.path.join(REPO, "scripts", "export_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--config", "c.yaml", "--ckpt", "x.ckpt", "--out", "m.ply"]
    a = cli.parse_args(base)
    assert a.min_component == 1 and a.largest is None and not a.fill_cavities
    b = cli.parse_args(base + ["--min-component", "50", "--largest", "3", "--fill-cavities"])
    assert b.min_component == 50 and b.largest == 3 and b.fill_cavities
    for bad in (["--min-component", "0"], ["--largest", "0"], ["--largest", "x"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)

"""GPU: the encoder's second input path in training -- unit positions stored once by the kernels that write the packed
sample stream, and the leading dense levels walked by one workgroup row -- against the ray-based, one-row-per-level path
(REN_KNOB_HG_VARIANT bit 3) in the same process.  Everything here is bit for bit (torch.equal): both paths run the same
helpers in the same order, so there is no tolerance to choose."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AABB6 = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
PER_LEVEL = 2 | 8                       # the knob's default (2) + one row per level for the dense levels too


@pytest.fixture(scope="module")
def amd():
    from robust_e_nerf_amd import ops, _lib
    _lib.load()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return ops


def make_rays(R, seed=0):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(R, generator=g) * 2 * math.pi
    o = torch.stack([4 * torch.cos(ang), 4 * torch.sin(ang), torch.rand(R, generator=g) - 0.5], -1)
    tgt = (torch.rand(R, 3, generator=g) - 0.5) * 2.0
    d = tgt - o
    d = d / d.norm(dim=-1, keepdim=True)
    return o.float().contiguous().to(DEV), d.float().contiguous().to(DEV)


def ball_binary(res, radius=1.1):
    lo, hi = np.array(AABB6[:3]), np.array(AABB6[3:])
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing="ij"), -1)
    c = (g + 0.5) / res * (hi - lo) + lo
    return torch.from_numpy(np.linalg.norm(c, axis=-1) < radius).to(torch.uint8).reshape(-1).to(DEV)


def crafted_stream(ops, counts, ct, seed=1):
    """a packed stream with the given per-ray counts, written -- with its unit positions -- by the sampler's cached write
    pass from intervals placed here: rays from radius 4 towards the box, t in [1, 7), so AABB positions fall on both sides
    of the unit cube's faces (the dense levels' index wrap runs)"""
    R, cap = len(counts), max(counts)
    o, d = make_rays(R, seed)
    g = torch.Generator().manual_seed(seed + 100)
    cache = torch.zeros(R, cap, 2)
    for r, c in enumerate(counts):
        t0 = torch.sort(1.0 + 6.0 * torch.rand(c, generator=g)).values
        cache[r, :c, 0] = t0
        cache[r, :c, 1] = t0 + 0.01 + 0.05 * torch.rand(c, generator=g)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    offsets, _ = ops.exclusive_scan(cnt)
    n = int(sum(counts))
    scene = ops.make_scene_desc(AABB6, ct)
    tmin, tmax = torch.zeros(R, device=DEV), torch.full((R,), 10.0, device=DEV)
    args = (o, d, tmin, tmax, None, AABB6, (32, 32, 32), ball_binary(32), ct, 0.01, 0.0, 0, 0)
    ri, ts, te, xu = ops.ray_march_write(*args, offsets, n, counts=cnt, cache=cache.to(DEV), unit_scene=scene)
    assert torch.equal(ts.cpu(), torch.cat([cache[r, :c, 0] for r, c in enumerate(counts)]))
    return dict(o=o, d=d, samples=(ri, ts, te), xu=xu, n=n, scene=scene)


def table_for(ops, grid, n_params, seed=3):
    return ((torch.rand(n_params, generator=torch.Generator().manual_seed(seed)) - 0.5) * 2.0).to(DEV)


def both_paths(ops, grid, table, s, layout, n=None, n_dev=None):
    """(ray-based + one row per level, unit positions + fused dense row) into buffers pre-filled alike"""
    n = s["n"] if n is None else n
    size = n * 2 * grid.n_levels if layout == 0 else ops.n_blocks32(n) * ops.FRAG_FLOATS_PER_BLOCK
    old, new = torch.full((size,), 7.0, device=DEV), torch.full((size,), 7.0, device=DEV)
    with ops.knob("hg_variant", PER_LEVEL):
        ops.hashgrid_fwd(grid, table, scene=s["scene"], rays=(s["o"], s["d"]), samples=s["samples"], n=n, layout=layout, out=old,
                         n_dev=n_dev)
    ops.hashgrid_fwd(grid, table, x_unit=s["xu"], n=n, layout=layout, out=new, n_dev=n_dev)
    torch.cuda.synchronize()
    return old, new


COUNTS = {1000: [100, 37, 200, 163, 1, 299, 200], 33: [20, 13]}


@pytest.mark.parametrize("ct", [0, 2], ids=["aabb", "sphere"])
@pytest.mark.parametrize("n", [1000, 33])
@pytest.mark.parametrize("layout", [0, 1])
def test_features_bit_identical(amd, layout, n, ct):
    ops = amd
    s = crafted_stream(ops, COUNTS[n], ct)
    assert s["n"] == n
    u = s["xu"].cpu()
    if ct == 0:
        assert bool(((u < 0) | (u > 1)).any()) and bool(((u > 0) & (u < 1)).all(dim=-1).any())
    grid, n_params = ops.make_grid_desc()
    old, new = both_paths(ops, grid, table_for(ops, grid, n_params), s, layout)
    assert bool((old != 7.0).all())                          # every entry written (layout 1: the padding lanes too)
    assert torch.equal(old, new)


@pytest.mark.parametrize("layout", [0, 1])
def test_device_count_below_capacity(amd, layout):
    """n_dev < capacity: the fragment padding follows the real count, and what lies beyond it is what the old path leaves"""
    ops = amd
    s = crafted_stream(ops, COUNTS[1000], 0)
    grid, n_params = ops.make_grid_desc()
    n_dev = torch.tensor([777], dtype=torch.int64, device=DEV)
    old, new = both_paths(ops, grid, table_for(ops, grid, n_params), s, layout, n_dev=n_dev)
    assert torch.equal(old, new)
    ref, _ = both_paths(ops, grid, table_for(ops, grid, n_params), s, layout, n=777)
    m = ref.numel() if layout == 1 else 777 * 32
    assert torch.equal(new[:m], ref[:m]) and bool((new[m:] == 7.0).all())


@pytest.mark.parametrize("kind", ["default", "all_hashed", "all_dense"])
def test_fused_dense_row_three_grids(amd, kind):
    """the mapping alone, both from the same input: 5 dense + 11 hashed levels, no dense level, nothing but dense levels"""
    ops = amd
    kw = dict(default={}, all_hashed=dict(log2_hashmap_size=11), all_dense=dict(n_levels=4, log2_hashmap_size=19))[kind]
    grid, n_params = ops.make_grid_desc(**kw)
    n_dense = sum(1 for l in range(grid.n_levels) if not grid.hashed[l])
    assert n_dense == dict(default=5, all_hashed=0, all_dense=4)[kind]
    s = crafted_stream(ops, COUNTS[1000], 0)
    table = table_for(ops, grid, n_params)
    for layout in ([0] if grid.n_levels != 16 else [0, 1]):
        for inp in (dict(x_unit=s["xu"]), dict(scene=s["scene"], rays=(s["o"], s["d"]), samples=s["samples"])):
            with ops.knob("hg_variant", PER_LEVEL):
                old = ops.hashgrid_fwd(grid, table, n=s["n"], layout=layout, **inp)
            new = ops.hashgrid_fwd(grid, table, n=s["n"], layout=layout, **inp)
            assert torch.equal(old, new)                     # (layout 1: the padding lanes of the last block are written too)


@pytest.mark.parametrize("ct", [0, 2], ids=["aabb", "sphere"])
def test_x_unit_of_the_uniform_write_kernel(amd, ct):
    ops = amd
    R, S = 64, 16
    o, d = make_rays(R, 5)
    scene = ops.make_scene_desc(AABB6, ct)
    tmin, tmax = ops.ray_aabb_intersect(o, d, AABB6, None, None)
    jit = torch.rand(R, generator=torch.Generator().manual_seed(6)).to(DEV)
    args = (o, d, tmin, tmax, jit, AABB6, (32, 32, 32), None, ct, 0.01, 0.0, 1, S)
    counts = ops.ray_march_count(*args)
    offsets, total = ops.exclusive_scan(counts)
    n = int(total.item())
    assert 0 < n <= R * S
    ri, ts, te, xu = ops.ray_march_write(*args, offsets, n, unit_scene=scene)
    ri0, ts0, te0 = ops.ray_march_write(*args, offsets, n)
    assert torch.equal(ri, ri0) and torch.equal(ts, ts0) and torch.equal(te, te0)
    assert torch.equal(xu, ops.unit_positions(scene, (o, d), (ri, ts, te), n))


@pytest.mark.parametrize("how", ["speculative", "sequential", "cached"])
def test_x_unit_of_the_march_write_pass(amd, how):
    """occupancy marcher, ball at 32^3: the speculative and the sequential write kernels, and the copy from the interval cache
    (cache of 4 intervals: longer rays are marched again, so both kernels of that pass write)"""
    ops = amd
    R = 64
    o, d = make_rays(R, 7)
    scene = ops.make_scene_desc(AABB6, 0)
    tmin, tmax = ops.ray_aabb_intersect(o, d, AABB6, None, None)
    jit = torch.rand(R, generator=torch.Generator().manual_seed(8)).to(DEV)
    args = (o, d, tmin, tmax, jit, AABB6, (32, 32, 32), ball_binary(32), 0, math.sqrt(3) * 3 / 256, 0.0, 0, 0)
    cache = torch.empty(R, 4, 2, device=DEV) if how == "cached" else None
    with ops.knob("march_sequential", 1 if how == "sequential" else 0):
        counts = ops.ray_march_count(*args, cache=cache)
        offsets, total = ops.exclusive_scan(counts)
        n = int(total.item())
        assert n > R and int(counts.max()) > 4 and int((counts > 0).sum()) > 8
        ri, ts, te, xu = ops.ray_march_write(*args, offsets, n, counts=counts, cache=cache, unit_scene=scene)
        ri0, ts0, te0 = ops.ray_march_write(*args, offsets, n, counts=counts, cache=cache)
    assert torch.equal(ri, ri0) and torch.equal(ts, ts0) and torch.equal(te, te0)
    assert torch.equal(xu, ops.unit_positions(scene, (o, d), (ri, ts, te), n))


def test_x_unit_moves_with_the_compacted_samples(amd):
    ops = amd
    counts = COUNTS[1000]
    s = crafted_stream(ops, counts, 0)
    ri, ts, te = s["samples"]
    keep = (torch.rand(s["n"], generator=torch.Generator().manual_seed(9)) < 0.6).to(torch.uint8)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    offsets, _ = ops.exclusive_scan(cnt)
    kept = torch.tensor([int(k.sum()) for k in torch.split(keep, counts)], dtype=torch.int32, device=DEV)
    new_offsets, total = ops.exclusive_scan(kept)
    n1 = int(total.item())
    ri2, ts2, te2, xu2 = ops.compact_samples(offsets, cnt, new_offsets, keep.to(DEV), ts, te, n1, x_unit=s["xu"])
    ri1, ts1, te1 = ops.compact_samples(offsets, cnt, new_offsets, keep.to(DEV), ts, te, n1)
    assert torch.equal(ri2, ri1) and torch.equal(ts2, ts1) and torch.equal(te2, te1)
    assert torch.equal(xu2, s["xu"][keep.bool().to(DEV)])
    assert torch.equal(xu2, ops.unit_positions(s["scene"], (s["o"], s["d"]), (ri2, ts2, te2), n1))

"""Surface normals, the parts that need no GPU: the colour code of a normal map, argument validation of
ren_hashgrid_bwd_input (bad arguments are refused before any launch) and the command-line flag."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normal_png_colour_code():
    from robust_e_nerf_amd import evaluation
    n = torch.zeros(3, 2, 4)
    n[:, 0, 0] = torch.tensor([1.0, 0.0, 0.0])
    n[:, 0, 1] = torch.tensor([0.0, -1.0, 0.0])
    n[:, 0, 2] = torch.tensor([0.0, 0.0, 0.25])           # any length: the code shows the direction
    n[:, 0, 3] = torch.tensor([-3.0, 0.0, 0.0])
    n[:, 1, 1] = torch.tensor([0.0, 1.0, 0.0])            # opacity 0: white whatever the vector
    n[:, 1, 2] = torch.tensor([1.0, 1.0, 1.0])
    opac = torch.ones(2, 4)
    opac[1, 1] = 0.0
    opac[1, 3] = 0.0
    u8 = evaluation.normal_png(n, opac)
    assert u8.dtype == torch.uint8 and u8.shape == (2, 4, 3) and u8.device.type == "cpu"
    assert u8[0, 0].tolist() == [255, 128, 128]
    assert u8[0, 1].tolist() == [128, 0, 128]
    assert u8[0, 2].tolist() == [128, 128, 255]
    assert u8[0, 3].tolist() == [0, 128, 128]
    assert u8[1, 0].tolist() == [128, 128, 128]           # a zero vector with opacity: mid grey, no NaN
    assert u8[1, 1].tolist() == [255, 255, 255] and u8[1, 3].tolist() == [255, 255, 255]
    c = round(255 * (1 / 3 ** 0.5 + 1) / 2)
    assert u8[1, 2].tolist() == [c, c, c]


def test_bwd_input_argument_validation_without_gpu():
    """null table, n < 0 and an unknown layout: REN_ERR_BAD_ARG -> ValueError, before any launch (the pointers are host
    memory and never read)"""
    from robust_e_nerf_amd import _lib, ops
    lib = _lib.load()
    grid, _ = ops.make_grid_desc()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(table=p, x_unit=p, n=4, layout=0, dfeat=p, dx=p, g=grid):
        return lib.ren_hashgrid_bwd_input(ctypes.byref(g) if g is not None else None, table, x_unit, None, None, None, None,
                                          None, None, n, layout, dfeat, dx, None)

    for kw in (dict(table=None), dict(n=-1), dict(layout=2), dict(layout=-1), dict(dfeat=None), dict(dx=None), dict(g=None),
               dict(x_unit=None)):                         # no x_unit and no sample stream either
        rc = call(**kw)
        assert rc == _lib.REN_ERR_BAD_ARG, kw
        with pytest.raises(ValueError):
            _lib.check(rc, "ren_hashgrid_bwd_input")
    assert call(n=0) == _lib.REN_OK                        # nothing to do, nothing launched
    assert lib.ren_abi_version() == 25                     # a new entry point changes no signature


def test_render_script_lists_normals_flag():
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "render.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--normals" in out.stdout

"""CPU: gp_field_score / gp_field_score_ws_bytes are declared, exported and bound, every argument
check answers on the host (LAPACK-style negative argument number) before any launch, the
workspace size is 0 for empty problems and monotone, and blas.field_score validates dtypes,
shapes, strides and devices of every operand before the call.

No device work happens here: the pointers handed over are never dereferenced.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpfit.h")
NAMES = ("gp_field_score", "gp_field_score_ws_bytes")


@pytest.fixture(scope="module")
def lib():
    from gladsgp_amd import _build, _capi
    _build.build_library()
    return _capi.lib()


def test_declared_exported_and_bound(lib):
    from gladsgp_amd import _build, _capi
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gp_[a-z_0-9]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gp_[a-z_0-9]+)", out))
    for name in NAMES:
        assert name in declared, name
        assert name in exported, name
        assert name in _capi.SIGNATURES, name
    assert len(_capi.SIGNATURES["gp_field_score"][1]) == 28
    assert len(_capi.SIGNATURES["gp_field_score_ws_bytes"][1]) == 4
    # the index names of the header and of the binding agree
    for pre, table in (("GPFIT_SCORE_ROW_", _capi.SCORE_ROW), ("GPFIT_SCORE_COL_", _capi.SCORE_COL)):
        named = {k.lower(): int(v) for k, v in re.findall(r"#define " + pre + r"(\w+) (\d+)", src)}
        assert named == table, (pre, named)
    assert sorted(_capi.SCORE_ROW.values()) == list(range(8))
    assert sorted(_capi.SCORE_COL.values()) == list(range(4))


# argument positions (1-based, the code returned is their negative)
(W, LDW, LDS, S, M, P, K, LDK, NCOLS, SD, MU, ERR, QLO, QHI, Y, LDY, YF32, FLOOR, MEAN, LO, HI,
 LDO, F32, ROWS, COLS, WS, WSB, STREAM) = range(1, 29)


def _args(**over):
    d = ctypes.c_void_p(64)
    a = {W: d, LDW: 8, LDS: 40, S: 64, M: 5, P: 8, K: d, LDK: 100, NCOLS: 100, SD: None, MU: None,
         ERR: None, QLO: 0.025, QHI: 0.975, Y: d, LDY: 100, YF32: 0, FLOOR: -np.inf, MEAN: None,
         LO: None, HI: None, LDO: 0, F32: 0, ROWS: d, COLS: d, WS: ctypes.c_void_p(256),
         WSB: 16, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 29)]


def test_base_arguments_stop_at_the_workspace_size(lib):
    """The base list is valid up to a workspace that is too small: nothing is launched."""
    assert lib.gp_field_score(*_args()) == -WSB


@pytest.mark.parametrize("over,code", [
    # gp_field_summary's checks, by the same numbers
    (dict(W=None), -W),
    (dict(LDW=7), -LDW),
    (dict(LDW=0, P=0), -LDW),
    (dict(LDS=39), -LDS),
    (dict(LDS=7, M=1), -LDS),
    (dict(S=0), -S),
    (dict(M=-1), -M),
    (dict(P=0), -P),
    (dict(P=65, LDW=65, LDS=400), -P),
    (dict(K=None), -K),
    (dict(LDK=99), -LDK),
    (dict(NCOLS=-1), -NCOLS),
    (dict(SD=ctypes.c_void_p(64)), -SD),
    (dict(MU=ctypes.c_void_p(64)), -SD),
    (dict(QLO=-0.1), -QLO),
    (dict(QLO=float("nan")), -QLO),
    (dict(QHI=1.5), -QHI),
    (dict(QLO=0.6, QHI=0.4, S=4), -QHI),
    (dict(QLO=0.2), -QLO),                     # S = 64: 14 order statistics > 8
    (dict(QHI=0.8), -QHI),
    (dict(S=512, QLO=0.0), -QHI),
    # the new arguments, each by its own number
    (dict(LDY=99), -LDY),
    (dict(LDY=0, NCOLS=0, LDK=1), -LDY),       # ldy < 1
    (dict(YF32=2), -YF32),
    (dict(MEAN=ctypes.c_void_p(64)), -LDO),    # an output is given: ldo counts
    (dict(LO=ctypes.c_void_p(64), LDO=99), -LDO),
    (dict(HI=ctypes.c_void_p(64), LDO=99), -LDO),
    (dict(F32=3), -F32),
    (dict(ROWS=None), -ROWS),
    (dict(WS=None), -WS),
    (dict(WS=ctypes.c_void_p(64)), -WS),       # not 256-B aligned
    (dict(WSB=0), -WSB),
    # order: the shared checks first, then the new ones as they are listed
    (dict(W=None, ROWS=None), -W),
    (dict(QLO=0.2, LDY=99), -QLO),
    (dict(LDY=99, YF32=2), -LDY),
    (dict(YF32=2, ROWS=None), -YF32),
    (dict(ROWS=None, WS=None), -ROWS),
    (dict(WS=None, WSB=0), -WS),
])
def test_argument_checks(lib, over, code):
    assert lib.gp_field_score(*_args(**over)) == code


def test_optional_arguments_and_empty_problems(lib):
    """Y, the three maps and cols may be NULL (then ldy / ldo are not looked at); a float32
    truth and float32 outputs pass; m = 0 or ncols = 0 returns 0 with no workspace at all."""
    for over in (dict(Y=None, LDY=0), dict(COLS=None), dict(YF32=1), dict(F32=1),
                 dict(MEAN=ctypes.c_void_p(64), LDO=100),
                 dict(MEAN=ctypes.c_void_p(64), LO=ctypes.c_void_p(64), HI=ctypes.c_void_p(64),
                      LDO=101),
                 dict(FLOOR=float("nan")), dict(FLOOR=float("inf"))):
        assert lib.gp_field_score(*_args(**over)) == -WSB, over
    assert lib.gp_field_score(*_args(M=0, LDS=8, WS=None, WSB=0)) == 0
    assert lib.gp_field_score(*_args(NCOLS=0, WS=None, WSB=0)) == 0
    assert lib.gp_field_score(*_args(M=0, LDS=8, ROWS=None)) == -ROWS   # still validated


def test_workspace_size(lib):
    f = lib.gp_field_score_ws_bytes
    assert f(64, 0, 8, 1000) == 0 and f(64, 5, 8, 0) == 0
    assert f(0, 5, 8, 100) == -1 and f(64, -1, 8, 100) == -1 and f(64, 5, 0, 100) == -1
    assert f(64, 5, 8, -1) == -1
    prev = 0
    for m in (1, 2, 3, 7, 100, 1000, 5000):
        cur = f(64, m, 8, 1000)
        assert cur >= prev and cur > 0 and cur % 256 == 0
        prev = cur
    assert f(64, 5000, 8, 1000) > f(64, 1, 8, 1000)
    prev = 0
    for n in (1, 127, 128, 129, 1000, 10_000, 1_347_945):
        cur = f(64, 100, 8, n)
        assert cur >= prev and cur > 0
        prev = cur
    assert f(64, 100, 8, 129) > f(64, 100, 8, 128)
    # the size does not depend on S or P, and the call accepts exactly it
    assert f(1, 100, 64, 1000) == f(64, 100, 8, 1000)
    need = f(64, 5, 8, 100)
    assert lib.gp_field_score(*_args(WSB=need - 1)) == -WSB
    # far below the three (m, ncols) float32 arrays it replaces at the reference's size
    assert f(64, 100, 8, 1_347_945) < 3 * 4 * 100 * 1_347_945 // 8


def _operands(S_=6, m=3, P_=4, ncols=10):
    g = torch.Generator().manual_seed(0)
    W3 = torch.randn((S_, m, P_), dtype=torch.float64, generator=g)
    Km = torch.randn((P_, ncols), dtype=torch.float64, generator=g)
    Y = torch.randn((m, ncols), dtype=torch.float64, generator=g)
    return W3, Km, Y


def test_field_score_validates_before_the_call():
    """Wrong dtypes, shapes, strides and devices raise ValueError from Python: nothing reaches
    the library (the operands are host tensors, which the last check refuses too)."""
    from gladsgp_amd import blas
    W3, Km, Y = _operands()
    S_, m, P_ = W3.shape
    ncols = Km.shape[1]
    f64 = torch.float64
    with pytest.raises(ValueError, match="field_score: K"):
        blas.field_score(W3, Km.float(), Y=Y)
    with pytest.raises(ValueError, match="W3"):
        blas.field_score(W3.float(), Km, Y=Y)
    with pytest.raises(ValueError, match="W3"):
        blas.field_score(W3[0], Km, Y=Y)
    with pytest.raises(ValueError):
        blas.field_score(W3, Km[:3], Y=Y)
    with pytest.raises(ValueError, match="stride"):
        blas.field_score(W3.transpose(1, 2).contiguous().transpose(1, 2), Km, Y=Y)
    with pytest.raises(ValueError, match="sample-major"):
        blas.field_score(W3.transpose(0, 1).contiguous().transpose(0, 1), Km, Y=Y)
    with pytest.raises(ValueError, match="row-major"):
        blas.field_score(W3, Km.t().contiguous().t(), Y=Y)
    with pytest.raises(ValueError, match="err"):
        blas.field_score(W3, Km, err=torch.zeros(S_ * m - 1, dtype=f64), Y=Y)
    with pytest.raises(ValueError, match="err"):
        blas.field_score(W3, Km, err=torch.zeros(S_ * m, dtype=torch.float32), Y=Y)
    with pytest.raises(ValueError, match="together"):
        blas.field_score(W3, Km, sd=torch.ones(ncols, dtype=f64), Y=Y)
    with pytest.raises(ValueError, match="mu"):
        blas.field_score(W3, Km, sd=torch.ones(ncols, dtype=f64),
                         mu=torch.zeros(ncols + 1, dtype=f64), Y=Y)
    with pytest.raises(ValueError, match="q_lo"):
        blas.field_score(W3, Km, Y=Y, q=(0.7, 0.2))
    # the truth
    with pytest.raises(ValueError, match="Y must be"):
        blas.field_score(W3, Km, Y=Y.numpy())
    with pytest.raises(ValueError, match="Y must be"):
        blas.field_score(W3, Km, Y=Y.to(torch.float16))
    with pytest.raises(ValueError, match="Y must be"):
        blas.field_score(W3, Km, Y=Y[:, :-1])
    with pytest.raises(ValueError, match="Y must be"):
        blas.field_score(W3, Km, Y=Y[:-1])
    with pytest.raises(ValueError, match="column stride"):
        blas.field_score(W3, Km, Y=Y.t().contiguous().t())
    with pytest.raises(ValueError, match="row stride"):
        blas.field_score(W3, Km, Y=Y[:1].expand(m, ncols))          # row stride 0
    with pytest.raises(ValueError, match="mape_floor"):
        blas.field_score(W3, Km, Y=Y, mape_floor="low")
    # the optional maps
    good = [torch.empty((m, ncols), dtype=f64) for _ in range(3)]
    with pytest.raises(ValueError, match="out"):
        blas.field_score(W3, Km, Y=Y, out=[good[0], good[1],
                                           torch.empty((m, ncols + 1), dtype=f64)])
    with pytest.raises(ValueError, match="out"):
        blas.field_score(W3, Km, Y=Y, out=good[:2])
    with pytest.raises(ValueError, match="out"):
        blas.field_score(W3, Km, Y=Y, f32=True, out=good)
    with pytest.raises(ValueError, match="row stride"):
        blas.field_score(W3, Km, Y=Y, out=[good[0], good[1],
                                           torch.empty((m, ncols + 2), dtype=f64)[:, :ncols]])
    # everything valid (a float32 truth with a padded row stride, maps, no truth), but on the host
    Y32 = torch.zeros((m, ncols + 3), dtype=torch.float32)[:, :ncols]
    for kw in (dict(Y=Y), dict(Y=Y32), dict(Y=None), dict(Y=Y, out=good), dict(Y=Y, cols=False)):
        with pytest.raises(ValueError, match="HIP device"):
            blas.field_score(W3, Km, **kw)

"""CPU: gp_pca_trunc and its three companions are declared, exported and bound, every argument
check answers on the host (LAPACK-style negative argument number) before any launch, the rank list
is validated, the workspace size is 0 for empty problems, -1 for bad ones and monotone, and
blas.pca_trunc validates dtypes, shapes, strides and devices of every operand before the call.

No device work happens here: the pointers handed over are never dereferenced.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpfit.h")
NAMES = ("gp_pca_trunc", "gp_pca_trunc_ws_bytes", "gp_pca_trunc_max_rank",
         "gp_pca_trunc_max_levels")


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
    assert len(_capi.SIGNATURES["gp_pca_trunc"][1]) == 19
    assert len(_capi.SIGNATURES["gp_pca_trunc_ws_bytes"][1]) == 3
    assert "pcatrunc.hip" in _build.SOURCES
    assert lib.gp_pca_trunc_max_rank() >= 128
    assert lib.gp_pca_trunc_max_levels() >= 32


# argument positions (1-based, the code returned is their negative)
(Y, LDY, YF32, N, NCOLS, MU, SD, C, LDC, V, LDV, RANKS, NLEV, TOT, NODE, LDN, WS, WSB,
 STREAM) = range(1, 20)


def _args(ranks=(1, 5, 8), **over):
    """A valid call up to a workspace that is too small; ``ranks``: the host list (None = NULL)."""
    d = ctypes.c_void_p(64)
    arr = (ctypes.c_int * max(len(ranks), 1))(*ranks) if ranks is not None else None
    a = {Y: d, LDY: 100, YF32: 1, N: 12, NCOLS: 100, MU: None, SD: None, C: d, LDC: 8, V: d,
         LDV: 100, RANKS: ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None,
         NLEV: len(ranks) if ranks is not None else 3, TOT: d, NODE: None, LDN: 0,
         WS: ctypes.c_void_p(256), WSB: 16, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 20)], arr         # arr: kept alive by the caller


def _call(lib, ranks=(1, 5, 8), **over):
    args, keep = _args(ranks, **over)
    return lib.gp_pca_trunc(*args)


def test_base_arguments_stop_at_the_workspace_size(lib):
    """The base list is valid up to a workspace that is too small: nothing is launched."""
    assert _call(lib) == -WSB


@pytest.mark.parametrize("over,code", [
    (dict(Y=None), -Y),
    (dict(LDY=99), -LDY),
    (dict(LDY=0, NCOLS=0, LDV=1), -LDY),        # ldy < 1
    (dict(YF32=2), -YF32),
    (dict(YF32=-1), -YF32),
    (dict(N=-1), -N),
    (dict(NCOLS=-1), -NCOLS),
    (dict(MU=ctypes.c_void_p(64)), -MU),        # one of the pair
    (dict(SD=ctypes.c_void_p(64)), -MU),
    (dict(C=None), -C),
    (dict(LDC=7), -LDC),                        # below pmax = 8
    (dict(V=None), -V),
    (dict(LDV=99), -LDV),
    (dict(NLEV=-1), -NLEV),
    (dict(TOT=None), -TOT),
    (dict(NODE=ctypes.c_void_p(64)), -LDN),     # node is given: ldn counts
    (dict(NODE=ctypes.c_void_p(64), LDN=99), -LDN),
    (dict(WS=None), -WS),
    (dict(WS=ctypes.c_void_p(64)), -WS),        # not 256-B aligned
    (dict(WSB=0), -WSB),
    # order: the sizes and the rank list first, then the operands as they are listed
    (dict(Y=None, N=-1), -N),
    (dict(N=-1, NCOLS=-1), -N),
    (dict(NCOLS=-1, NLEV=-1), -NCOLS),
    (dict(Y=None, NLEV=-1), -NLEV),
    (dict(Y=None, LDY=99), -Y),
    (dict(LDY=99, YF32=2), -LDY),
    (dict(YF32=2, MU=ctypes.c_void_p(64)), -YF32),
    (dict(MU=ctypes.c_void_p(64), C=None), -MU),
    (dict(C=None, LDC=7), -C),
    (dict(LDC=7, V=None), -LDC),
    (dict(LDV=99, TOT=None), -LDV),
    (dict(TOT=None, NODE=ctypes.c_void_p(64)), -TOT),
    (dict(NODE=ctypes.c_void_p(64), WS=None), -LDN),
    (dict(WS=None, WSB=0), -WS),
])
def test_argument_checks(lib, over, code):
    assert _call(lib, **over) == code


def test_rank_list_checks(lib):
    """Ranks are strictly increasing within [0, max_rank]; nlev <= max_levels; a NULL list is
    refused when there are levels; every refusal is -RANKS / -NLEV and comes before the
    operands' checks."""
    mr, ml = lib.gp_pca_trunc_max_rank(), lib.gp_pca_trunc_max_levels()
    wide = dict(LDC=mr)
    for bad in ((3, 3), (5, 4), (1, 2, 2), (-1, 2), (0, 0), (1, mr + 1), (mr + 1,)):
        assert _call(lib, ranks=bad, **wide) == -RANKS, bad
        assert _call(lib, ranks=bad, Y=None, **wide) == -RANKS, bad
    assert _call(lib, ranks=None) == -RANKS
    for good in ((0,), (0, 1, 2, 3, 4, 5), (mr,), (1, mr), tuple(range(1, ml + 1)),
                 tuple(range(mr - ml + 1, mr + 1))):
        assert _call(lib, ranks=good, **wide) == -WSB, good
    too_many = tuple(range(1, ml + 2))
    assert _call(lib, ranks=too_many, **wide) == -NLEV
    assert _call(lib, ranks=(1, 5, 8), LDC=8) == -WSB         # ldc is measured against pmax
    assert _call(lib, ranks=(1, 5, 9), LDC=8) == -LDC


def test_optional_arguments_and_empty_problems(lib):
    """mu / sd may be NULL together or both given, node may be NULL (then ldn is not looked at),
    an fp64 Y passes; n = 0, ncols = 0 or nlev = 0 return 0 with no workspace at all, after the
    same validation."""
    p = ctypes.c_void_p(64)
    for over in (dict(MU=p, SD=p), dict(YF32=0), dict(NODE=p, LDN=100), dict(NODE=p, LDN=117),
                 dict(LDY=131), dict(LDV=101), dict(LDC=9)):
        assert _call(lib, **over) == -WSB, over
    assert _call(lib, N=0, WS=None, WSB=0) == 0
    assert _call(lib, NCOLS=0, WS=None, WSB=0) == 0
    assert _call(lib, ranks=(), NLEV=0, WS=None, WSB=0) == 0
    assert _call(lib, ranks=None, NLEV=0, WS=None, WSB=0) == 0
    assert _call(lib, N=0, TOT=None) == -TOT                  # still validated
    assert _call(lib, NCOLS=0, C=None) == -C
    assert _call(lib, ranks=(2, 1), N=0) == -RANKS


def test_workspace_size(lib):
    f = lib.gp_pca_trunc_ws_bytes
    ml = lib.gp_pca_trunc_max_levels()
    assert f(0, 1000, 3) == 0 and f(12, 0, 3) == 0 and f(12, 1000, 0) == 0
    assert f(-1, 1000, 3) == -1 and f(12, -1, 3) == -1 and f(12, 1000, -1) == -1
    assert f(12, 1000, ml + 1) == -1
    prev = 0
    for ncols in (1, 63, 64, 65, 1000, 100_000, 1_347_945):
        cur = f(512, ncols, 26)
        assert cur >= prev and cur > 0 and cur % 256 == 0
        prev = cur
    assert f(512, 1_347_945, 26) > f(512, 1000, 26)
    prev = 0
    for nlev in range(1, ml + 1):
        cur = f(512, 100_000, nlev)
        assert cur >= prev and cur > 0 and cur % 256 == 0
        prev = cur
    assert f(512, 100_000, ml) > f(512, 100_000, 1)
    assert f(1, 1000, 3) == f(512, 1000, 3)                   # the rows are walked, not stored
    need = f(12, 100, 3)
    assert _call(lib, WSB=need - 1) == -WSB
    # far below one (n, ncols) fp64 residual at the reference's size
    assert f(512, 1_347_945, 26) < 8 * 512 * 1_347_945 // 100


def _operands(n=6, ncols=10, p=4):
    g = torch.Generator().manual_seed(0)
    Yt = torch.randn((n, ncols), dtype=torch.float64, generator=g)
    Ct = torch.randn((n, p), dtype=torch.float64, generator=g)
    Vt = torch.randn((p, ncols), dtype=torch.float64, generator=g)
    return Yt, Ct, Vt


def test_pca_trunc_validates_before_the_call():
    """Wrong dtypes, shapes, strides, rank lists and devices raise ValueError from Python: nothing
    reaches the library (the operands are host tensors, which the last check refuses too)."""
    from gladsgp_amd import blas
    Yt, Ct, Vt = _operands()
    n, ncols = Yt.shape
    p = Ct.shape[1]
    f64 = torch.float64
    rk = [1, 3]
    # dtypes
    with pytest.raises(ValueError, match="pca_trunc: Y"):
        blas.pca_trunc(Yt.to(torch.float16), Ct, Vt, rk)
    with pytest.raises(ValueError, match="pca_trunc: Y"):
        blas.pca_trunc(Yt.numpy(), Ct, Vt, rk)
    with pytest.raises(ValueError, match="pca_trunc: C"):
        blas.pca_trunc(Yt, Ct.float(), Vt, rk)
    with pytest.raises(ValueError, match="pca_trunc: V"):
        blas.pca_trunc(Yt, Ct, Vt.float(), rk)
    # shapes
    with pytest.raises(ValueError, match="pca_trunc: Y"):
        blas.pca_trunc(Yt[0], Ct, Vt, rk)
    with pytest.raises(ValueError, match="needs C"):
        blas.pca_trunc(Yt, Ct[:-1], Vt, rk)
    with pytest.raises(ValueError, match="needs C"):
        blas.pca_trunc(Yt, Ct, Vt[:-1], rk)
    with pytest.raises(ValueError, match="needs C"):
        blas.pca_trunc(Yt, Ct, Vt[:, :-1], rk)
    # strides: a column stride != 1, a row stride of 0
    with pytest.raises(ValueError, match="Y needs a unit column stride"):
        blas.pca_trunc(Yt.t().contiguous().t(), Ct, Vt, rk)
    with pytest.raises(ValueError, match="C needs a unit column stride"):
        blas.pca_trunc(Yt, Ct.t().contiguous().t(), Vt, rk)
    with pytest.raises(ValueError, match="V needs a unit column stride"):
        blas.pca_trunc(Yt, Ct, Vt.t().contiguous().t(), rk)
    with pytest.raises(ValueError, match="Y needs a row stride"):
        blas.pca_trunc(Yt[:1].expand(n, ncols), Ct, Vt, rk)
    with pytest.raises(ValueError, match="V needs a row stride"):
        blas.pca_trunc(Yt, Ct, Vt[:1].expand(p, ncols), rk)
    # mu / sd
    with pytest.raises(ValueError, match="together"):
        blas.pca_trunc(Yt, Ct, Vt, rk, mu=torch.zeros(ncols, dtype=f64))
    with pytest.raises(ValueError, match="together"):
        blas.pca_trunc(Yt, Ct, Vt, rk, sd=torch.ones(ncols, dtype=f64))
    with pytest.raises(ValueError, match="pca_trunc: sd has"):
        blas.pca_trunc(Yt, Ct, Vt, rk, mu=torch.zeros(ncols, dtype=f64),
                       sd=torch.ones(ncols + 1, dtype=f64))
    with pytest.raises(ValueError, match="pca_trunc: mu must"):
        blas.pca_trunc(Yt, Ct, Vt, rk, mu=torch.zeros(ncols, dtype=torch.float32),
                       sd=torch.ones(ncols, dtype=f64))
    with pytest.raises(ValueError, match="pca_trunc: sd must"):
        blas.pca_trunc(Yt, Ct, Vt, rk, mu=torch.zeros(ncols, dtype=f64),
                       sd=torch.ones(2 * ncols, dtype=f64)[::2])
    # ranks
    for bad in ([], [2, 2], [3, 1], [-1, 2], [1.5], [1, p + 1], "ab"):
        with pytest.raises(ValueError, match="pca_trunc: rank"):
            blas.pca_trunc(Yt, Ct, Vt, bad)
    # out
    tot = torch.empty((2, 2), dtype=f64)
    nod = torch.empty((2, ncols), dtype=f64)
    with pytest.raises(ValueError, match="out"):
        blas.pca_trunc(Yt, Ct, Vt, rk, out=(tot,))
    with pytest.raises(ValueError, match="tot"):
        blas.pca_trunc(Yt, Ct, Vt, rk, out=(torch.empty((3, 2), dtype=f64), None))
    with pytest.raises(ValueError, match="node"):
        blas.pca_trunc(Yt, Ct, Vt, rk, node=True, out=(tot, None))
    with pytest.raises(ValueError, match="node"):
        blas.pca_trunc(Yt, Ct, Vt, rk, node=False, out=(tot, nod))
    with pytest.raises(ValueError, match="node"):
        blas.pca_trunc(Yt, Ct, Vt, rk, node=True, out=(tot, nod[:, :-1]))
    with pytest.raises(ValueError, match="node needs a unit column stride"):
        blas.pca_trunc(Yt, Ct, Vt, rk, node=True,
                       out=(tot, torch.empty((ncols, 2), dtype=f64).t()))
    # everything valid (float32 ensemble with a padded row stride, statistics, node), but on the host
    Y32 = torch.zeros((n, ncols + 3), dtype=torch.float32)[:, :ncols]
    mu, sd = torch.zeros(ncols, dtype=f64), torch.ones(ncols, dtype=f64)
    for args, kw in (((Yt, Ct, Vt, rk), {}), ((Y32, Ct, Vt, [0, p]), dict(mu=mu, sd=sd)),
                     ((Yt, Ct, Vt, rk), dict(node=True)),
                     ((Yt, Ct, Vt, rk), dict(node=True, out=(tot, nod)))):
        with pytest.raises(ValueError, match="HIP device"):
            blas.pca_trunc(*args, **kw)

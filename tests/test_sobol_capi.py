"""CPU: gp_sobol_replicates / gp_sobol_lds_points are declared, exported and bound, every argument
check answers on the host (LAPACK-style negative argument number) before any launch, and
sensitivity.sobol_replicates validates dtypes, shapes, strides and device before the call.

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
NAMES = ("gp_sobol_replicates", "gp_sobol_lds_points")


@pytest.fixture(scope="module")
def lib():
    from gladsgp_amd import _build, _capi
    _build.build_library()
    return _capi.lib()


def test_declared_exported_and_bound(lib):
    from gladsgp_amd import _build, _capi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(gp_[a-z_0-9]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gp_[a-z_0-9]+)", out))
    for name in NAMES:
        assert name in declared, name
        assert name in exported, name
        assert name in _capi.SIGNATURES, name
    assert len(_capi.SIGNATURES["gp_sobol_replicates"][1]) == 24
    assert "sobol.hip" in _build.SOURCES
    for k, name in enumerate(("IDENTITY", "INDEX", "PHILOX", "JACKKNIFE")):
        assert re.search(rf"#define GPFIT_SOBOL_{name} {k}\b", src)


def test_lds_points(lib):
    from gladsgp_amd import sensitivity
    assert lib.gp_sobol_lds_points(0) == 0
    assert lib.gp_sobol_lds_points(33) == 0                      # d > GPFIT_MAX_DIM
    pts = [lib.gp_sobol_lds_points(d) for d in range(1, 33)]
    assert all(a >= b for a, b in zip(pts, pts[1:]))
    assert pts[7] >= 256                                         # the reference's case is resident
    assert pts[0] <= 1 << 20
    assert sensitivity.lds_points(8) == pts[7]


# argument positions (1-based, the code returned is their negative)
(FA, FB, FAB, LDF, STRIDEAB, N, P, D, MODE, IDX, LDI, NDRAW, R, SEED, OFFSET, PCVAR, CLAMP, FIRST,
 TOTAL, LDR, GFIRST, GTOTAL, LDG, STREAM) = range(1, 25)
IDENTITY, INDEX, PHILOX, JACKKNIFE = range(4)
PTR = ctypes.c_void_p(64)


def _args(**over):
    a = {FA: PTR, FB: PTR, FAB: PTR, LDF: 16, STRIDEAB: 48, N: 16, P: 3, D: 2, MODE: INDEX,
         IDX: PTR, LDI: 16, NDRAW: 16, R: 4, SEED: 1, OFFSET: 0, PCVAR: None, CLAMP: 0, FIRST: PTR,
         TOTAL: PTR, LDR: 6, GFIRST: None, GTOTAL: None, LDG: 0, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 25)]


# every case fails one check, so nothing is ever launched on the made-up pointers
@pytest.mark.parametrize("over,code", [
    (dict(FA=None), -FA),
    (dict(FB=None), -FB),
    (dict(FAB=None), -FAB),
    (dict(LDF=15), -LDF),
    (dict(STRIDEAB=47), -STRIDEAB),                    # < (p - 1) ldf + N
    (dict(LDF=20, STRIDEAB=55), -STRIDEAB),
    (dict(N=1, NDRAW=1), -N),
    (dict(N=(1 << 20) + 1, LDF=1 << 21, STRIDEAB=1 << 23), -N),
    (dict(P=0), -P),
    (dict(D=0), -D),
    (dict(D=33, LDR=99), -D),                          # d > GPFIT_MAX_DIM
    (dict(MODE=-1), -MODE),
    (dict(MODE=4), -MODE),
    (dict(IDX=None), -IDX),                            # INDEX without rows
    (dict(LDI=15), -LDI),
    (dict(NDRAW=0), -NDRAW),
    (dict(MODE=PHILOX, NDRAW=0), -NDRAW),
    (dict(MODE=IDENTITY, R=1, NDRAW=15), -NDRAW),      # IDENTITY: n_draw = N
    (dict(MODE=IDENTITY, R=2), -R),                    # IDENTITY: R = 1
    (dict(MODE=IDENTITY, R=0), -R),
    (dict(MODE=JACKKNIFE, R=16, NDRAW=16), -NDRAW),    # JACKKNIFE: n_draw = N - 1
    (dict(MODE=JACKKNIFE, R=15, NDRAW=15), -R),        # JACKKNIFE: R = N
    (dict(R=-1), -R),
    (dict(GFIRST=PTR), -PCVAR),                        # the trio goes together
    (dict(GTOTAL=PTR), -PCVAR),
    (dict(PCVAR=PTR, LDG=2), -GFIRST),
    (dict(PCVAR=PTR, GFIRST=PTR, LDG=2), -GTOTAL),
    (dict(PCVAR=PTR, GFIRST=PTR, GTOTAL=PTR, LDG=1), -LDG),
    (dict(FIRST=None), -FIRST),
    (dict(TOTAL=None), -TOTAL),
    (dict(LDR=5), -LDR),
    (dict(MODE=IDENTITY, R=1, IDX=None, FIRST=None), -FIRST),        # no rows needed
    (dict(MODE=JACKKNIFE, R=16, NDRAW=15, IDX=None, FIRST=None), -FIRST),
    (dict(MODE=PHILOX, IDX=None, NDRAW=1000, FIRST=None), -FIRST),   # n_draw is free
])
def test_argument_checks(lib, over, code):
    assert lib.gp_sobol_replicates(*_args(**over)) == code


def test_no_replicates_is_a_no_op(lib):
    assert lib.gp_sobol_replicates(*_args(R=0)) == 0
    assert lib.gp_sobol_replicates(*_args(R=0, MODE=PHILOX, IDX=None)) == 0
    assert lib.gp_sobol_replicates(*_args(R=0, PCVAR=PTR, GFIRST=PTR, GTOTAL=PTR, LDG=2)) == 0
    assert lib.gp_sobol_replicates(*_args(R=0, LDR=5)) == -LDR       # still validated


def test_sobol_replicates_validates_before_the_call():
    """Wrong dtypes, shapes, strides and modes raise ValueError from Python: nothing reaches the
    library (the operands are host tensors, which the last check refuses too)."""
    from gladsgp_amd import sensitivity as sn
    g = torch.Generator().manual_seed(0)
    p, n, d = 3, 10, 2
    fA = torch.randn((p, n), dtype=torch.float64, generator=g)
    fB = torch.randn((p, n), dtype=torch.float64, generator=g)
    fAB = torch.randn((d, p, n), dtype=torch.float64, generator=g)
    idx = torch.zeros((4, n), dtype=torch.int32)
    with pytest.raises(ValueError, match="fA"):
        sn.sobol_replicates(fA.float(), fB, fAB)
    with pytest.raises(ValueError, match="fAB"):
        sn.sobol_replicates(fA, fB, fAB[0])
    with pytest.raises(ValueError, match="fB"):
        sn.sobol_replicates(fA, fB[:, :9], fAB)
    with pytest.raises(ValueError, match="N"):
        sn.sobol_replicates(fA[:, :1], fB[:, :1], fAB[:, :, :1])
    with pytest.raises(ValueError, match="unit last stride"):
        sn.sobol_replicates(fA.t().contiguous().t(), fB, fAB)
    with pytest.raises(ValueError, match="row stride"):
        sn.sobol_replicates(torch.zeros((p, n + 2), dtype=torch.float64)[:, :n], fB, fAB)
    with pytest.raises(ValueError, match="input stride"):
        sn.sobol_replicates(fA, fB, fAB.flip(0).flip(0).as_strided((d, p, n), (n, n, 1)))
    with pytest.raises(ValueError, match="mode"):
        sn.sobol_replicates(fA, fB, fAB, mode=7)
    with pytest.raises(ValueError, match="mode"):
        sn.sobol_replicates(fA, fB, fAB, mode="bootstrap")
    with pytest.raises(ValueError, match="IDENTITY"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.IDENTITY, R=2)
    with pytest.raises(ValueError, match="JACKKNIFE"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.JACKKNIFE, n_draw=n)
    with pytest.raises(ValueError, match="R is required"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.PHILOX)
    with pytest.raises(ValueError, match="idx"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.INDEX, idx=idx.long())
    with pytest.raises(ValueError, match="idx"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.INDEX, idx=idx, n_draw=n - 1)
    with pytest.raises(ValueError, match="idx"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.INDEX)
    with pytest.raises(ValueError, match="idx"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.PHILOX, R=3, idx=idx)
    with pytest.raises(ValueError, match="pcvar"):
        sn.sobol_replicates(fA, fB, fAB, pcvar=torch.ones(p + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="pcvar"):
        sn.sobol_replicates(fA, fB, fAB, pcvar=torch.ones(p))
    with pytest.raises(ValueError, match="HIP device"):
        sn.sobol_replicates(fA, fB, fAB, mode=sn.INDEX, idx=idx)    # all valid, but on the host

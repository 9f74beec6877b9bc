"""CPU: gp_field_summary / gp_field_summary_max_tail are declared, exported and bound, and every
argument check answers on the host (LAPACK-style negative argument number) before any launch;
blas.field_summary validates dtypes, shapes and strides of every operand before the call.

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
NAMES = ("gp_field_summary", "gp_field_summary_max_tail")


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
    assert len(_capi.SIGNATURES["gp_field_summary"][1]) == 20
    assert "summary.hip" in _build.SOURCES


def test_max_tail_is_eight(lib):
    from gladsgp_amd import blas
    assert lib.gp_field_summary_max_tail() == 8
    assert blas.field_summary_max_tail() == 8


# argument positions (1-based, the code returned is their negative)
W, LDW, LDS, S, M, P, K, LDK, NCOLS, SD, MU, ERR, QLO, QHI, MEAN, LO, HI, LDO, F32, STREAM = \
    range(1, 21)


def _args(**over):
    d = ctypes.c_void_p(64)
    a = {W: d, LDW: 8, LDS: 40, S: 64, M: 5, P: 8, K: d, LDK: 100, NCOLS: 100, SD: None, MU: None,
         ERR: None, QLO: 0.025, QHI: 0.975, MEAN: d, LO: d, HI: d, LDO: 100, F32: 0, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 21)]


@pytest.mark.parametrize("over,code", [
    (dict(W=None), -W),
    (dict(LDW=7), -LDW),                       # ldw < P
    (dict(LDW=0, P=0), -LDW),                  # ldw < 1 (before P is looked at)
    (dict(LDS=39), -LDS),                      # lds < (m - 1) ldw + P
    (dict(LDS=7, M=1), -LDS),                  # lds < P
    (dict(S=0), -S),
    (dict(M=-1), -M),
    (dict(P=0), -P),
    (dict(P=65, LDW=65, LDS=400), -P),         # P > gp_field_max_pcs()
    (dict(K=None), -K),
    (dict(LDK=99), -LDK),
    (dict(NCOLS=-1), -NCOLS),
    (dict(SD=ctypes.c_void_p(64)), -SD),       # sd without mu
    (dict(MU=ctypes.c_void_p(64)), -SD),       # mu without sd
    (dict(QLO=-0.1), -QLO),
    (dict(QLO=float("nan")), -QLO),
    (dict(QHI=1.5), -QHI),
    (dict(QLO=0.6, QHI=0.4, S=4), -QHI),       # q_lo > q_hi
    (dict(QLO=0.2), -QLO),                     # S = 64: floor(0.2 * 63) + 2 = 14 > 8
    (dict(QHI=0.8), -QHI),                     # S = 64: 64 - floor(0.8 * 63) = 14 > 8
    (dict(S=512, QLO=0.0), -QHI),              # 512 - floor(0.975 * 511) = 14 > 8
    (dict(MEAN=None), -MEAN),                  # q = 0.025 at S = 64 passed validation
    (dict(LO=None), -LO),
    (dict(HI=None), -HI),
    (dict(LDO=99), -LDO),
])
def test_argument_checks(lib, over, code):
    assert lib.gp_field_summary(*_args(**over)) == code


def test_depth_rule(lib):
    """The reference's settings fit: q = 0.025 needs depth 2 / 3 / 5 at S = 32 / 64 / 128; any q
    fits while S <= 8; a valid call on an empty problem is a no-op."""
    from gladsgp_amd import blas
    for s_, depth in ((32, 2), (64, 3), (128, 5)):
        assert max(blas.summary_tail_depths(s_, 0.025, 1 - 0.025)) == depth
        assert lib.gp_field_summary(*_args(S=s_, MEAN=None)) == -MEAN      # past the q checks
    assert lib.gp_field_summary(*_args(S=8, QLO=0.5, QHI=0.5, MEAN=None)) == -MEAN
    assert lib.gp_field_summary(*_args(S=9, QLO=1.0, QHI=1.0, MEAN=None)) == -QLO  # 9 smallest
    assert lib.gp_field_summary(*_args(QLO=0.0, QHI=1.0, MEAN=None)) == -MEAN      # min / max
    assert lib.gp_field_summary(*_args(M=0, LDS=8)) == 0
    assert lib.gp_field_summary(*_args(NCOLS=0)) == 0


def _operands(S_=6, m=3, P_=4, ncols=10):
    g = torch.Generator().manual_seed(0)
    W3 = torch.randn((S_, m, P_), dtype=torch.float64, generator=g)
    Km = torch.randn((P_, ncols), dtype=torch.float64, generator=g)
    return W3, Km


def test_field_summary_validates_before_the_call():
    """Wrong dtypes, shapes and strides raise ValueError from Python: nothing reaches the
    library (the operands are host tensors, which the last check refuses too)."""
    from gladsgp_amd import blas
    W3, Km = _operands()
    S_, m, P_ = W3.shape
    ncols = Km.shape[1]
    f64 = torch.float64
    with pytest.raises(ValueError, match="K"):
        blas.field_summary(W3, Km.float())
    with pytest.raises(ValueError, match="W3"):
        blas.field_summary(W3.float(), Km)
    with pytest.raises(ValueError, match="W3"):
        blas.field_summary(W3[0], Km)
    with pytest.raises(ValueError):
        blas.field_summary(W3, Km[:3])                              # K rows != P
    with pytest.raises(ValueError, match="stride"):
        blas.field_summary(W3.transpose(1, 2).contiguous().transpose(1, 2), Km)
    with pytest.raises(ValueError, match="sample-major"):
        blas.field_summary(W3.transpose(0, 1).contiguous().transpose(0, 1), Km)
    with pytest.raises(ValueError, match="row-major"):
        blas.field_summary(W3, Km.t().contiguous().t())
    with pytest.raises(ValueError, match="err"):
        blas.field_summary(W3, Km, err=torch.zeros(S_ * m - 1, dtype=f64))
    with pytest.raises(ValueError, match="err"):
        blas.field_summary(W3, Km, err=torch.zeros(S_ * m, dtype=torch.float32))
    with pytest.raises(ValueError, match="together"):
        blas.field_summary(W3, Km, sd=torch.ones(ncols, dtype=f64))
    with pytest.raises(ValueError, match="sd"):
        blas.field_summary(W3, Km, sd=torch.ones(ncols + 1, dtype=f64),
                           mu=torch.zeros(ncols, dtype=f64))
    with pytest.raises(ValueError, match="q_lo"):
        blas.field_summary(W3, Km, q=(0.7, 0.2))
    good = [torch.empty((m, ncols), dtype=f64) for _ in range(3)]
    with pytest.raises(ValueError, match="out"):
        blas.field_summary(W3, Km, out=[good[0], good[1], torch.empty((m, ncols + 1), dtype=f64)])
    with pytest.raises(ValueError, match="out"):
        blas.field_summary(W3, Km, out=good[:2])
    with pytest.raises(ValueError, match="out"):
        blas.field_summary(W3, Km, f32=True, out=good)              # dtype follows f32
    with pytest.raises(ValueError, match="row stride"):
        blas.field_summary(W3, Km, out=[good[0], good[1],
                                        torch.empty((m, ncols + 2), dtype=f64)[:, :ncols]])
    with pytest.raises(ValueError, match="column stride"):
        blas.field_summary(W3, Km, out=[torch.empty((ncols, m), dtype=f64).t() for _ in range(3)])
    with pytest.raises(ValueError, match="HIP device"):
        blas.field_summary(W3, Km, out=good)                        # all valid, but on the host

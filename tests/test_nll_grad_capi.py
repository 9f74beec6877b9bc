"""CPU: gp_nll_grad / gp_nll_grad_ws_bytes are declared, exported and bound, every argument check
answers on the host (LAPACK-style negative argument number) before any launch, and
kernels.nll_grad / kernels.nll_value_grad validate dtype, shape, contiguity and device before the
call.

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
NAMES = ("gp_nll_grad", "gp_nll_grad_ws_bytes")


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
    assert len(_capi.SIGNATURES["gp_nll_grad"][1]) == 18
    assert len(_capi.SIGNATURES["gp_nll_grad_ws_bytes"][1]) == 3
    assert "nllgrad.hip" in _build.SOURCES


(LINV, LDINV, STRIDE, X, LDX, N, D, BETA, LDBETA, S, ALPHA, LDA, GRAD, LDG, BATCH, WS, WSB,
 STREAM) = range(1, 19)
_NPAD = 128
_P = ctypes.c_void_p(256)
MAX_DIM = 32                                    # GPFIT_MAX_DIM


def _args(**over):
    """A valid call (n = 100, d = 8, batch 2) up to its null workspace."""
    a = {LINV: _P, LDINV: _NPAD, STRIDE: _NPAD * _NPAD, X: _P, LDX: 8, N: 100, D: 8, BETA: _P,
         LDBETA: 8, S: _P, ALPHA: _P, LDA: 100, GRAD: _P, LDG: 10, BATCH: 2, WS: None,
         WSB: 1 << 40, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 19)]


@pytest.mark.parametrize("over,code", [
    (dict(), -WS),                              # the base list is valid up to its null workspace
    (dict(LINV=None), -LINV),
    (dict(LDINV=_NPAD - 1), -LDINV),            # ldinv < gp_padded_n(n)
    (dict(LDINV=100), -LDINV),
    (dict(STRIDE=_NPAD * _NPAD - 1), -STRIDE),
    (dict(STRIDE=0, BATCH=1), -WS),             # one problem: no stride to check
    (dict(X=None), -X),
    (dict(LDX=7), -LDX),                        # ldx < d
    (dict(N=-1), -N),
    (dict(D=0), -D),
    (dict(D=MAX_DIM + 1, LDX=40, LDBETA=40, LDG=40), -D),
    (dict(D=MAX_DIM, LDX=32, LDBETA=32, LDG=34), -WS),
    (dict(BETA=None), -BETA),
    (dict(LDBETA=7), -LDBETA),
    (dict(LDBETA=0, BATCH=1), -WS),             # ldbeta is a batch stride
    (dict(S=None), -S),
    (dict(ALPHA=None), -ALPHA),
    (dict(LDA=99), -LDA),
    (dict(LDA=0, BATCH=1), -WS),
    (dict(GRAD=None), -GRAD),
    (dict(LDG=9), -LDG),                        # ldg < d + 2
    (dict(LDG=9, BATCH=1), -LDG),
    (dict(BATCH=-1), -BATCH),
    (dict(WS=ctypes.c_void_p(16)), -WS),        # workspace not 256-B aligned
    (dict(WS=_P, WSB=16), -WSB),
    # odd ld, odd stride, 8-B base: accepted (alignment only selects wider loads)
    (dict(LINV=ctypes.c_void_p(8), LDINV=_NPAD + 1, STRIDE=(_NPAD + 1) * _NPAD + 1), -WS),
    (dict(N=0), 0), (dict(BATCH=0), 0),         # no-ops
    (dict(N=0, LDINV=1, STRIDE=0), 0),
    (dict(N=0, GRAD=None), -GRAD),              # ... after the checks
])
def test_argument_checks(lib, over, code):
    assert lib.gp_nll_grad(*_args(**over)) == code


def test_workspace_size(lib):
    f = lib.gp_nll_grad_ws_bytes
    # one 64 x 64 lower tile per block, d + 2 partial sums each
    assert f(64, 8, 1) == 256 and f(65, 8, 1) == 256
    assert f(512, 8, 1) == 3072                 # 36 tiles x 10 sums x 8 bytes, in 256-B units
    assert f(512, 8, 3) >= 3 * 36 * 10 * 8 and f(512, 8, 3) % 256 == 0
    sizes = [f(n, 8, 2) for n in (1, 64, 65, 129, 512, 513, 4096)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert f(300, 1, 2) < f(300, 32, 2)
    assert f(0, 8, 4) == 0 and f(512, 8, 0) == 0
    assert f(-1, 8, 1) == -1 and f(1, -1, 1) == -1 and f(1, 8, -1) == -1
    # one byte less than the exact size is refused (the exact size would launch: a GPU test's)
    assert lib.gp_nll_grad(*_args(WS=_P, WSB=f(100, 8, 2) - 1)) == -WSB


def _chol(batch=2, n=10):
    from gladsgp_amd import kernels
    npad = kernels.padded_n(n)
    return kernels.Cholesky(n, torch.zeros((batch, n, n), dtype=torch.float64),
                            torch.zeros((batch, npad, npad), dtype=torch.float64),
                            torch.zeros(batch, dtype=torch.int32),
                            torch.zeros(batch, dtype=torch.float64))


def test_nll_grad_validates_before_the_call():
    from gladsgp_amd import kernels
    f64 = torch.float64
    ch = _chol()
    X, beta, s = torch.zeros((10, 3), dtype=f64), torch.zeros((2, 3), dtype=f64), \
        torch.zeros(2, dtype=f64)
    w = torch.zeros((2, 10), dtype=f64)
    ng = kernels.nll_grad
    with pytest.raises(ValueError, match="^chol"):
        ng(ch.linv_buf, X, beta, s, w)
    with pytest.raises(ValueError, match="^w"):
        ng(ch, X, beta, s, w.float())
    with pytest.raises(ValueError, match="^w.*shape"):
        ng(ch, X, beta, s, torch.zeros((2, 9), dtype=f64))
    with pytest.raises(ValueError, match="^w.*contiguous"):
        ng(ch, X, beta, s, torch.zeros((10, 2), dtype=f64).t())
    with pytest.raises(ValueError, match="^X"):
        ng(ch, X.float(), beta, s, w)
    with pytest.raises(ValueError, match="^X.*shape"):
        ng(ch, torch.zeros((9, 3), dtype=f64), beta, s, w)
    with pytest.raises(ValueError, match="^X.*contiguous"):
        ng(ch, torch.zeros((3, 10), dtype=f64).t(), beta, s, w)
    with pytest.raises(ValueError, match="^beta.*shape"):
        ng(ch, X, torch.zeros((2, 4), dtype=f64), s, w)
    with pytest.raises(ValueError, match="^beta.*contiguous"):
        ng(ch, X, torch.zeros((3, 2), dtype=f64).t(), s, w)
    with pytest.raises(ValueError, match="^s:"):
        ng(ch, X, beta, torch.zeros(3, dtype=f64), w)
    with pytest.raises(ValueError, match="^alpha.*shape"):
        ng(ch, X, beta, s, w, alpha=torch.zeros((2, 11), dtype=f64))
    with pytest.raises(ValueError, match="^alpha"):
        ng(ch, X, beta, s, w, alpha=w.float())
    with pytest.raises(ValueError, match="HIP device"):
        ng(ch, X, beta, s, w, alpha=w)                      # all valid, but on the host


def test_nll_value_grad_validates_before_the_call():
    from gladsgp_amd import kernels
    f64 = torch.float64
    X, beta = torch.zeros((10, 3), dtype=f64), torch.zeros((2, 3), dtype=f64)
    s, delta, w = torch.zeros(2, dtype=f64), torch.zeros(2, dtype=f64), \
        torch.zeros((2, 10), dtype=f64)
    vg = kernels.nll_value_grad
    with pytest.raises(ValueError, match="^X"):
        vg(X.float(), beta, s, delta, w)
    with pytest.raises(ValueError, match="^beta.*shape"):
        vg(X, torch.zeros((2, 4), dtype=f64), s, delta, w)
    with pytest.raises(ValueError, match="^s:"):
        vg(X, beta, torch.zeros(3, dtype=f64), delta, w)
    with pytest.raises(ValueError, match="^delta"):
        vg(X, beta, s, delta.float(), w)
    with pytest.raises(ValueError, match="^w.*shape"):
        vg(X, beta, s, delta, torch.zeros((2, 9), dtype=f64))
    with pytest.raises(ValueError, match="^w.*contiguous"):
        vg(X, beta, s, delta, torch.zeros((10, 2), dtype=f64).t())
    with pytest.raises(ValueError, match="HIP device"):
        vg(X, beta, s, delta, w)                            # all valid, but on the host

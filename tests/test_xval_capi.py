"""CPU: gp_xval / gp_xval_ws_bytes / gp_xval_max_fold are declared, exported and bound, every
argument check answers on the host (LAPACK-style negative argument number) before any launch, and
kernels.xval validates folds, dtypes and contiguity before the call.

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
NAMES = ("gp_xval", "gp_xval_ws_bytes", "gp_xval_max_fold")


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
    assert len(_capi.SIGNATURES["gp_xval"][1]) == 19
    assert "xval.hip" in _build.SOURCES
    assert "#define GPFIT_XVAL_MAX_FOLD 64" in open(HEADER).read()


def test_max_fold_is_64(lib):
    from gladsgp_amd import kernels
    assert lib.gp_xval_max_fold() == 64
    assert kernels.xval_max_fold() == 64


# argument positions (1-based, the code returned is their negative)
(LINV, LDINV, STRIDE, N, W, LDW, PTR, IDX, NFOLDS, NIDX, SHIFT, MEAN, VAR, LDO, INFO, BATCH, WS,
 WSB, STREAM) = range(1, 20)
_NPAD = 128


def _args(**over):
    d = ctypes.c_void_p(256)
    a = {LINV: d, LDINV: _NPAD, STRIDE: _NPAD * _NPAD, N: 100, W: d, LDW: 100, PTR: d, IDX: d,
         NFOLDS: 3, NIDX: 70, SHIFT: None, MEAN: d, VAR: d, LDO: 100, INFO: None, BATCH: 2,
         WS: None, WSB: 1 << 40, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 20)]


@pytest.mark.parametrize("over,code", [
    (dict(), -WS),                              # the base list is valid up to its null workspace
    (dict(LINV=None), -LINV),
    (dict(LDINV=_NPAD - 1), -LDINV),            # ldinv < gp_padded_n(n)
    (dict(LDINV=100), -LDINV),
    (dict(STRIDE=_NPAD * _NPAD - 1), -STRIDE),
    (dict(STRIDE=0, BATCH=1), -WS),             # one problem: no stride to check
    (dict(N=-1), -N),
    (dict(W=None), -W),
    (dict(LDW=99), -LDW),
    (dict(LDW=0, BATCH=1), -WS),                # ldw is a batch stride
    (dict(PTR=None), -PTR),                     # one fold pointer without the other
    (dict(IDX=None), -IDX),
    (dict(NFOLDS=-1), -NFOLDS),
    (dict(PTR=None, IDX=None), -NFOLDS),        # the NULL form wants nfolds = nidx = 0
    (dict(PTR=None, IDX=None, NFOLDS=0), -NIDX),
    (dict(PTR=None, IDX=None, NFOLDS=0, NIDX=0), -WS),
    (dict(NIDX=-1), -NIDX),
    (dict(NIDX=101), -NIDX),                    # nidx > n
    (dict(MEAN=None), -MEAN),
    (dict(VAR=None), -VAR),
    (dict(LDO=99), -LDO),
    (dict(LDO=0, BATCH=1), -WS),
    (dict(BATCH=-1), -BATCH),
    (dict(WS=ctypes.c_void_p(16)), -WS),        # workspace not 256-B aligned
    (dict(WS=ctypes.c_void_p(256), WSB=16), -WSB),
    (dict(LINV=ctypes.c_void_p(8), LDINV=_NPAD + 1, STRIDE=(_NPAD + 1) * _NPAD + 1), -WS),
    (dict(N=0, NIDX=0), 0), (dict(BATCH=0), 0),  # no-ops
    (dict(N=0), -NIDX),                         # ... after the checks: nidx > n
    (dict(N=0, LDINV=1, STRIDE=0, NIDX=0), 0),
])
def test_argument_checks(lib, over, code):
    assert lib.gp_xval(*_args(**over)) == code


def test_workspace_size(lib):
    one = lib.gp_xval_ws_bytes(512, 0, 0, 1)
    assert one >= 8 * 512
    assert lib.gp_xval_ws_bytes(512, 0, 0, 8) > one
    assert lib.gp_xval_ws_bytes(512, 8, 512, 8) >= 8 * 8 * 512
    assert lib.gp_xval_ws_bytes(0, 0, 0, 4) == 0
    assert lib.gp_xval_ws_bytes(512, 0, 0, 0) == 0
    assert lib.gp_xval_ws_bytes(-1, 0, 0, 1) == -1
    # exactly enough passes the size check (and stops at nothing else: folds given, none to run)
    wsp = ctypes.c_void_p(256)
    assert lib.gp_xval(*_args(WS=wsp, WSB=lib.gp_xval_ws_bytes(100, 0, 70, 2), NFOLDS=0)) == 0
    assert lib.gp_xval(*_args(WS=wsp, WSB=lib.gp_xval_ws_bytes(100, 0, 70, 2) - 1,
                              NFOLDS=0)) == -WSB


def _chol(batch=2, n=10):
    from gladsgp_amd import kernels
    npad = kernels.padded_n(n)
    return kernels.Cholesky(n, torch.zeros((batch, n, n), dtype=torch.float64),
                            torch.zeros((batch, npad, npad), dtype=torch.float64),
                            torch.zeros(batch, dtype=torch.int32),
                            torch.zeros(batch, dtype=torch.float64))


def test_xval_validates_before_the_call():
    """Bad folds, dtypes and strides raise ValueError naming the argument; nothing reaches the
    library (the operands are host tensors, which the last check refuses too)."""
    from gladsgp_amd import kernels
    ch = _chol()
    w = torch.zeros((2, 10), dtype=torch.float64)
    with pytest.raises(ValueError, match="folds.*twice"):
        kernels.xval(ch, w, folds=[[0, 1], [2, 1]])
    with pytest.raises(ValueError, match="folds.*outside"):
        kernels.xval(ch, w, folds=[[0, 10]])
    with pytest.raises(ValueError, match="folds.*outside"):
        kernels.xval(ch, w, folds=[[-1]])
    big = _chol(1, 100)
    with pytest.raises(ValueError, match="folds.*65"):
        kernels.xval(big, torch.zeros((1, 100), dtype=torch.float64), folds=[list(range(65))])
    with pytest.raises(ValueError, match="^w"):
        kernels.xval(ch, w.float())
    with pytest.raises(ValueError, match="^w.*contiguous"):
        kernels.xval(ch, torch.zeros((10, 2), dtype=torch.float64).t())
    with pytest.raises(ValueError, match="^w.*shape"):
        kernels.xval(ch, torch.zeros((2, 9), dtype=torch.float64))
    with pytest.raises(ValueError, match="^shift"):
        kernels.xval(ch, w, shift=torch.zeros(2, dtype=torch.float32))
    with pytest.raises(ValueError, match="^shift"):
        kernels.xval(ch, w, shift=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="^out"):
        kernels.xval(ch, w, out=(torch.zeros((2, 10), dtype=torch.float64),))
    with pytest.raises(ValueError, match="^out"):
        kernels.xval(ch, w, out=(torch.zeros((2, 10), dtype=torch.float64),
                                 torch.zeros((2, 11), dtype=torch.float64)))
    with pytest.raises(ValueError, match="^chol"):
        kernels.xval(ch.linv_buf, w)
    with pytest.raises(ValueError, match="HIP device"):
        kernels.xval(ch, w, folds=[[0, 1], [5]])        # all valid, but on the host

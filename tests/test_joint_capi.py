"""CPU: gp_predict_cov / gp_predict_cov_ws_bytes / gp_mvn_draw are declared, exported and bound,
and every argument check answers on the host, in argument order, before any launch (minus the
argument's position; the workspace of gp_predict_cov with gp_predict's codes -21 / -22).

No device work happens here: the pointers handed over are never dereferenced.
"""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpfit.h")
NAMES = ("gp_predict_cov", "gp_predict_cov_ws_bytes", "gp_mvn_draw")


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
        assert name in declared and name in exported and name in _capi.SIGNATURES, name
    assert len(_capi.SIGNATURES["gp_predict_cov"][1]) == 22
    assert len(_capi.SIGNATURES["gp_mvn_draw"][1]) == 14
    assert "jointcov.hip" in _build.SOURCES
    from gladsgp_amd import kernels
    assert issubclass(kernels.JointNotPositiveDefinite, ValueError)


# ------------------------------------------------------------------------------ gp_predict_cov
(LINV, LDINV, STRIDE, X, LDX, XS, LDXS, N, M, D, BETA, LDBETA, S, SPRED, JITTER, C, LDC, STRIDEC,
 BATCH, WS, WSB, STREAM) = range(1, 23)
WS_NULL, WS_SMALL = -21, -22          # the workspace codes (gp_predict's)
_NPAD = 128
_P = ctypes.c_void_p(256)


def _cov_args(**over):
    """A valid call of 2 problems, n = 100, m = 40, d = 3 -- up to its null workspace."""
    a = {LINV: _P, LDINV: _NPAD, STRIDE: _NPAD * _NPAD, X: _P, LDX: 3, XS: _P, LDXS: 3, N: 100,
         M: 40, D: 3, BETA: _P, LDBETA: 3, S: _P, SPRED: _P, JITTER: None, C: _P, LDC: 40,
         STRIDEC: 1600, BATCH: 2, WS: None, WSB: 1 << 40, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 23)]


@pytest.mark.parametrize("over,code", [
    (dict(), WS_NULL),                           # the base list is valid up to its workspace
    (dict(LINV=None), -LINV),
    (dict(LINV=ctypes.c_void_p(8)), -LINV),      # gp_predict's contract: 16-B aligned
    (dict(LDINV=_NPAD - 2), -LDINV),             # ldinv < gp_padded_n(n)
    (dict(LDINV=_NPAD + 1), -LDINV),             # odd
    (dict(STRIDE=_NPAD * _NPAD - 2), -STRIDE),
    (dict(STRIDE=_NPAD * _NPAD + 1), -STRIDE),   # odd
    (dict(STRIDE=0, BATCH=1), WS_NULL),          # one problem: no stride to check
    (dict(X=None), -X),
    (dict(LDX=2), -LDX),
    (dict(XS=None), -XS),
    (dict(LDXS=2), -LDXS),
    (dict(N=-1), -N),
    (dict(M=-1), -M),
    (dict(D=0, LDX=0, LDXS=0, LDBETA=0), -D),
    (dict(D=33, LDX=33, LDXS=33, LDBETA=33), -D),
    (dict(D=32, LDX=32, LDXS=32, LDBETA=32), WS_NULL),
    (dict(BETA=None), -BETA),
    (dict(LDBETA=2), -LDBETA),
    (dict(LDBETA=0, BATCH=1), WS_NULL),          # ldbeta is a batch stride
    (dict(S=None), -S),
    (dict(SPRED=None), -SPRED),
    (dict(JITTER=_P), WS_NULL),                  # jitter is optional
    (dict(C=None), -C),
    (dict(LDC=39), -LDC),
    (dict(STRIDEC=1599), -STRIDEC),
    (dict(STRIDEC=0, BATCH=1), WS_NULL),
    (dict(BATCH=-1), -BATCH),
    (dict(WS=ctypes.c_void_p(16)), WS_NULL),     # workspace not 256-B aligned
    (dict(WS=_P, WSB=16), WS_SMALL),
    (dict(M=0), 0), (dict(BATCH=0), 0),          # no-ops
    (dict(M=0, C=None), -C),                     # ... after the checks
    # the order of the checks: the earliest argument answers
    (dict(LINV=None, X=None, C=None, BATCH=-1), -LINV),
    (dict(LDINV=1, X=None), -LDINV),
    (dict(X=None, XS=None, N=-1), -X),
    (dict(N=-1, M=-1, D=0), -N),
    (dict(M=-1, BETA=None), -M),
    (dict(S=None, SPRED=None, C=None), -S),
    (dict(C=None, LDC=0, BATCH=-1), -C),
    (dict(LDC=1, BATCH=-1), -LDC),
    (dict(BATCH=-1, WS=_P, WSB=0), -BATCH),
    (dict(WS=ctypes.c_void_p(16), WSB=0), WS_NULL),
])
def test_predict_cov_argument_checks(lib, over, code):
    assert lib.gp_predict_cov(*_cov_args(**over)) == code


def test_predict_cov_workspace_size(lib):
    f = lib.gp_predict_cov_ws_bytes
    one = f(512, 512, 1)
    # K* (gp_padded_n(n) rows) and V (n rows), k-major rows of m test points
    assert one >= 8 * (512 + 512) * 512 and one % 256 == 0
    sizes = [f(300, 70, b) for b in (1, 2, 3, 64, 1000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 5
    assert f(300, 70, 1000) >= 1000 * 8 * 300 * 70 * 2
    assert [f(n, 33, 3) for n in (1, 17, 129, 513)] == sorted(f(n, 33, 3) for n in (1, 17, 129, 513))
    assert [f(64, m, 3) for m in (1, 64, 65, 257)] == sorted(f(64, m, 3) for m in (1, 64, 65, 257))
    assert f(0, 4, 4) == 0 and f(4, 0, 4) == 0 and f(4, 4, 0) == 0
    assert f(-1, 1, 1) == -1 and f(1, -1, 1) == -1 and f(1, 1, -1) == -1
    # one byte less than the exact size is refused (the exact size would launch: a GPU test's)
    assert lib.gp_predict_cov(*_cov_args(WS=_P, WSB=f(100, 40, 2) - 1)) == WS_SMALL


# --------------------------------------------------------------------------------- gp_mvn_draw
(R, LDR, STRIDER, DM, MEAN, LDM, NSAMP, SEED, OFFSET, UNIT0, OUT, LDO, DBATCH, DSTREAM) = \
    range(1, 15)


def _draw_args(**over):
    """Valid for 2 problems of m = 40 and 3 draws -- with nsamp = 0, so nothing is launched."""
    a = {R: _P, LDR: 40, STRIDER: 1600, DM: 40, MEAN: _P, LDM: 40, NSAMP: 0, SEED: 7, OFFSET: 0,
         UNIT0: 0, OUT: _P, LDO: 40, DBATCH: 2, DSTREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 15)]


@pytest.mark.parametrize("over,code", [
    (dict(), 0),
    (dict(R=None), -R),
    (dict(LDR=39), -LDR),
    (dict(LDR=0, DM=0), -LDR),
    (dict(STRIDER=1599), -STRIDER),
    (dict(STRIDER=0, DBATCH=1), 0),
    (dict(DM=-1), -DM),
    (dict(MEAN=None, LDM=0), 0),                 # mean is optional
    (dict(LDM=39), -LDM),
    (dict(LDM=0, DBATCH=1), 0),
    (dict(NSAMP=-1), -NSAMP),
    (dict(NSAMP=(1 << 18) + 1), -NSAMP),
    (dict(UNIT0=-1), -UNIT0),
    (dict(OUT=None), -OUT),
    (dict(LDO=39), -LDO),
    (dict(DBATCH=-1), -DBATCH),
    (dict(DM=0, LDR=1), 0), (dict(DBATCH=0), 0),
    (dict(DBATCH=0, OUT=None), -OUT),            # no-ops come after the checks
    (dict(R=None, DM=-1, OUT=None), -R),         # the earliest argument answers
    (dict(DM=-1, NSAMP=-1), -DM),
    (dict(NSAMP=-1, UNIT0=-1, OUT=None), -NSAMP),
    (dict(UNIT0=-1, OUT=None), -UNIT0),
    (dict(OUT=None, LDO=0, DBATCH=-1), -OUT),
    (dict(LDO=0, DBATCH=-1), -LDO),
])
def test_mvn_draw_argument_checks(lib, over, code):
    assert lib.gp_mvn_draw(*_draw_args(**over)) == code

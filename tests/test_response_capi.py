"""CPU: gp_alpha / gp_alpha_ws_bytes / gp_mean_response and its two limits are declared, exported
and bound, every argument check answers on the host (LAPACK-style negative argument number)
before any launch, and kernels.alpha / kernels.mean_response validate dtype, shape, contiguity
and device before the call.

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
NAMES = ("gp_alpha", "gp_alpha_ws_bytes", "gp_mean_response", "gp_mean_response_max_grid",
         "gp_mean_response_max_int_elems")


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
    assert len(_capi.SIGNATURES["gp_alpha"][1]) == 12
    assert len(_capi.SIGNATURES["gp_mean_response"][1]) == 25
    assert "response.hip" in _build.SOURCES
    for line in ("#define GPFIT_RESP_CYCLIC 0", "#define GPFIT_RESP_ASCENDING 1",
                 "#define GPFIT_RESP_MAX_EFFECTS 64"):
        assert line in text, line


def test_limits(lib):
    from gladsgp_amd import kernels
    assert lib.gp_mean_response_max_grid() == 64
    assert lib.gp_mean_response_max_int_elems() >= 2048
    assert kernels.mean_response_max_grid() == 64
    assert kernels.mean_response_max_int_elems() == lib.gp_mean_response_max_int_elems()
    assert kernels.RESP_MAX_EFFECTS == 64
    assert kernels.RESP_ORDER == {"cyclic": 0, "ascending": 1}


# ------------------------------------------------------------------------------------ gp_alpha
(LINV, LDINV, STRIDE, N, W, LDW, ALPHA, LDA, BATCH, WS, WSB, STREAM) = range(1, 13)
_NPAD = 128
_D = ctypes.c_void_p(256)


def _alpha_args(**over):
    a = {LINV: _D, LDINV: _NPAD, STRIDE: _NPAD * _NPAD, N: 100, W: _D, LDW: 100, ALPHA: _D,
         LDA: 100, BATCH: 2, WS: None, WSB: 1 << 40, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 13)]


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
    (dict(ALPHA=None), -ALPHA),
    (dict(LDA=99), -LDA),
    (dict(LDA=0, BATCH=1), -WS),
    (dict(BATCH=-1), -BATCH),
    (dict(WS=ctypes.c_void_p(16)), -WS),        # workspace not 256-B aligned
    (dict(WS=_D, WSB=16), -WSB),
    (dict(LINV=ctypes.c_void_p(8), LDINV=_NPAD + 1, STRIDE=(_NPAD + 1) * _NPAD + 1), -WS),
    (dict(N=0), 0), (dict(BATCH=0), 0),         # no-ops
    (dict(N=0, LDINV=1, STRIDE=0), 0),
    (dict(N=0, ALPHA=None), -ALPHA),            # ... after the checks
])
def test_alpha_argument_checks(lib, over, code):
    assert lib.gp_alpha(*_alpha_args(**over)) == code


def test_alpha_workspace_size(lib):
    one = lib.gp_alpha_ws_bytes(512, 1)
    assert one >= 8 * 512 and one % 256 == 0
    sizes = [lib.gp_alpha_ws_bytes(n, 3) for n in (1, 17, 128, 129, 512, 513, 2000)]
    assert sizes == sorted(sizes)
    sizes = [lib.gp_alpha_ws_bytes(300, b) for b in (1, 2, 3, 64, 1000)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert lib.gp_alpha_ws_bytes(0, 4) == 0
    assert lib.gp_alpha_ws_bytes(512, 0) == 0
    assert lib.gp_alpha_ws_bytes(-1, 1) == -1 and lib.gp_alpha_ws_bytes(1, -1) == -1
    # one byte less than the exact size is refused (the exact size would launch: a GPU test's)
    assert lib.gp_alpha(*_alpha_args(WS=_D, WSB=lib.gp_alpha_ws_bytes(100, 2) - 1)) == -WSB


# ---------------------------------------------------------------------------- gp_mean_response
(X, RN, RD, LDX, AL, RLDA, BETA, LDBETA, S, RBATCH, EFFECTS, NFREE, E, ORDER, T1P, T1, T2P, T2,
 XINT, I, LDI, OUT, LDE, LDB, RSTREAM) = range(1, 26)
CYCLIC, ASCENDING = 0, 1
_MAIN = (ctypes.c_int * 3)(0, 3, 7)
_PAIRS = (ctypes.c_int * 4)(0, 3, 7, 2)


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _resp_args(**over):
    """A valid pair call: d = 8, two pairs, 11 x 11 grids, 10 integration points, batch 2 -- up
    to n = 0 (nothing is launched: the pointers are never dereferenced)."""
    a = {X: _D, RN: 0, RD: 8, LDX: 8, AL: _D, RLDA: 100, BETA: _D, LDBETA: 8, S: _D, RBATCH: 2,
         EFFECTS: _PAIRS, NFREE: 2, E: 2, ORDER: ASCENDING, T1P: _D, T1: 11, T2P: _D, T2: 11,
         XINT: _D, I: 10, LDI: 6, OUT: _D, LDE: 121, LDB: 242, RSTREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 26)]


_MAINCALL = dict(EFFECTS=_MAIN, NFREE=1, E=3, T2P=None, T2=0, LDI=7, LDE=11, LDB=33)


@pytest.mark.parametrize("over,code", [
    (dict(), 0),                                            # n = 0: validated, nothing launched
    (dict(RN=100, RBATCH=0), 0), (dict(RN=100, E=0), 0),    # the other no-ops
    (dict(RN=100, E=0, EFFECTS=None), 0),
    (dict(**_MAINCALL), 0),
    (dict(_MAINCALL, ORDER=CYCLIC), 0),
    (dict(X=None), -X),
    (dict(RN=-1), -RN),
    (dict(RD=0), -RD), (dict(RD=33, LDX=33, LDBETA=33), -RD),
    (dict(LDX=7), -LDX),
    (dict(AL=None), -AL),
    (dict(RN=101), -RLDA),                                  # lda < n
    (dict(BETA=None), -BETA),
    (dict(LDBETA=7), -LDBETA),
    (dict(S=None), -S),
    (dict(RBATCH=-1), -RBATCH),
    (dict(EFFECTS=None), -EFFECTS),
    (dict(EFFECTS=_ints(0, 3, 7, 8)), -EFFECTS),            # a dimension outside [0, d)
    (dict(EFFECTS=_ints(0, 3, -1, 2)), -EFFECTS),
    (dict(EFFECTS=_ints(0, 3, 5, 5)), -EFFECTS),            # d1 == d2
    (dict(_MAINCALL, EFFECTS=_ints(0, 8, 1)), -EFFECTS),
    (dict(NFREE=0), -NFREE), (dict(NFREE=3), -NFREE),
    (dict(RD=1, LDX=1, LDBETA=1), -NFREE),                  # pairs of a one-dimensional design
    (dict(E=-1), -E),
    (dict(E=65), -E),                                       # above GPFIT_RESP_MAX_EFFECTS
    (dict(ORDER=2), -ORDER), (dict(ORDER=-1), -ORDER),
    (dict(ORDER=CYCLIC), -ORDER),                           # the main effects' rule with pairs
    (dict(T1P=None), -T1P),
    (dict(T1=0), -T1), (dict(T1=65, LDE=65 * 11, LDB=2 * 65 * 11), -T1),
    (dict(T2P=None), -T2P),
    (dict(T2=0), -T2), (dict(T2=65, LDE=65 * 11, LDB=2 * 65 * 11), -T2),
    (dict(_MAINCALL, T2=99), 0),                            # t2 / T2 ignored for main effects
    (dict(XINT=None), -XINT),
    (dict(I=0), -I),
    (dict(I=342), -I),                                      # 342 * 6 > 2048
    (dict(I=341), 0),
    (dict(LDI=5), -LDI),
    (dict(_MAINCALL, LDI=6), -LDI),
    (dict(RD=2, LDX=2, LDBETA=2, EFFECTS=_ints(0, 1, 1, 0), XINT=None, I=0, LDI=0), 0),
    (dict(_MAINCALL, RD=1, LDX=1, LDBETA=1, EFFECTS=_ints(0, 0, 0), XINT=None, I=-5,
          LDI=0), 0),                                       # d == nfree: Xint NULL, I ignored
    (dict(OUT=None), -OUT),
    (dict(LDE=120), -LDE),
    (dict(_MAINCALL, LDE=10), -LDE),
    (dict(LDB=241), -LDB),
    (dict(LDE=130, LDB=250), -LDB),                         # (E - 1) lde + T1 T2 = 251
    (dict(LDE=130, LDB=251), 0),
    (dict(RLDA=0, LDBETA=0, RBATCH=1, RN=0), 0),            # one problem: no batch strides
])
def test_mean_response_argument_checks(lib, over, code):
    assert lib.gp_mean_response(*_resp_args(**over)) == code


def _chol(batch=2, n=10):
    from gladsgp_amd import kernels
    npad = kernels.padded_n(n)
    return kernels.Cholesky(n, torch.zeros((batch, n, n), dtype=torch.float64),
                            torch.zeros((batch, npad, npad), dtype=torch.float64),
                            torch.zeros(batch, dtype=torch.int32),
                            torch.zeros(batch, dtype=torch.float64))


def test_alpha_validates_before_the_call():
    from gladsgp_amd import kernels
    ch = _chol()
    w = torch.zeros((2, 10), dtype=torch.float64)
    with pytest.raises(ValueError, match="^chol"):
        kernels.alpha(ch.linv_buf, w)
    with pytest.raises(ValueError, match="^w"):
        kernels.alpha(ch, w.float())
    with pytest.raises(ValueError, match="^w.*shape"):
        kernels.alpha(ch, torch.zeros((2, 9), dtype=torch.float64))
    with pytest.raises(ValueError, match="^w.*contiguous"):
        kernels.alpha(ch, torch.zeros((10, 2), dtype=torch.float64).t())
    with pytest.raises(ValueError, match="^out"):
        kernels.alpha(ch, w, out=torch.zeros((2, 11), dtype=torch.float64))
    with pytest.raises(ValueError, match="^out"):
        kernels.alpha(ch, w, out=torch.zeros((2, 10), dtype=torch.float32))
    with pytest.raises(ValueError, match="^out"):
        kernels.alpha(ch, w, out=torch.zeros((2, 20), dtype=torch.float64)[:, ::2])
    with pytest.raises(ValueError, match="HIP device"):
        kernels.alpha(ch, w)                                # all valid, but on the host


def test_mean_response_validates_before_the_call():
    """Every ValueError names its argument; nothing reaches the library (the operands are host
    tensors, which the last check refuses too)."""
    from gladsgp_amd import kernels
    f64 = torch.float64
    X = torch.zeros((10, 4), dtype=f64)
    al = torch.zeros((2, 10), dtype=f64)
    beta = torch.zeros((2, 4), dtype=f64)
    s = torch.zeros(2, dtype=f64)
    t = torch.zeros(11, dtype=f64)
    Xm, Xp = torch.zeros((20, 3), dtype=f64), torch.zeros((10, 2), dtype=f64)
    mr = kernels.mean_response
    with pytest.raises(ValueError, match="^X"):
        mr(X.float(), al, beta, s, [0], t, Xint=Xm)
    with pytest.raises(ValueError, match="^X.*contiguous"):
        mr(torch.zeros((4, 10), dtype=f64).t(), al, beta, s, [0], t, Xint=Xm)
    with pytest.raises(ValueError, match="^alpha.*shape"):
        mr(X, torch.zeros((2, 9), dtype=f64), beta, s, [0], t, Xint=Xm)
    with pytest.raises(ValueError, match="^alpha"):
        mr(X, al.float(), beta, s, [0], t, Xint=Xm)
    with pytest.raises(ValueError, match="^beta.*shape"):
        mr(X, al, torch.zeros((2, 3), dtype=f64), s, [0], t, Xint=Xm)
    with pytest.raises(ValueError, match="^beta.*contiguous"):
        mr(X, al, torch.zeros((4, 2), dtype=f64).t(), s, [0], t, Xint=Xm)
    with pytest.raises(ValueError, match="^s:"):
        mr(X, al, beta, torch.zeros(3, dtype=f64), [0], t, Xint=Xm)
    with pytest.raises(ValueError, match="^effects.*outside"):
        mr(X, al, beta, s, [0, 4], t, Xint=Xm)
    with pytest.raises(ValueError, match="^effects.*outside"):
        mr(X, al, beta, s, [(0, -1)], t, t, Xint=Xp)
    with pytest.raises(ValueError, match="^effects.*twice"):
        mr(X, al, beta, s, [(2, 2)], t, t, Xint=Xp)
    with pytest.raises(ValueError, match="^effects"):
        mr(X, al, beta, s, [(0, 1, 2)], t, t, Xint=Xp)
    with pytest.raises(ValueError, match="^effects"):
        mr(X, al, beta, s, [0.5], t, Xint=Xm)
    with pytest.raises(ValueError, match="^order"):
        mr(X, al, beta, s, [0], t, Xint=Xm, order="random")
    with pytest.raises(ValueError, match="^order.*cyclic"):
        mr(X, al, beta, s, [(0, 1)], t, t, Xint=Xp, order="cyclic")
    with pytest.raises(ValueError, match="^t1"):
        mr(X, al, beta, s, [0], torch.zeros(65, dtype=f64), Xint=Xm)
    with pytest.raises(ValueError, match="^t1"):
        mr(X, al, beta, s, [0], torch.zeros(0, dtype=f64), Xint=Xm)
    with pytest.raises(ValueError, match="^t1"):
        mr(X, al, beta, s, [0], t.float(), Xint=Xm)
    with pytest.raises(ValueError, match="^t2"):
        mr(X, al, beta, s, [(0, 1)], t, None, Xint=Xp)
    with pytest.raises(ValueError, match="^t2"):
        mr(X, al, beta, s, [(0, 1)], t, torch.zeros(65, dtype=f64), Xint=Xp)
    with pytest.raises(ValueError, match="^t2"):
        mr(X, al, beta, s, [0], t, t, Xint=Xm)
    with pytest.raises(ValueError, match="^Xint"):
        mr(X, al, beta, s, [0], t)
    with pytest.raises(ValueError, match="^Xint.*shape"):
        mr(X, al, beta, s, [0], t, Xint=Xp)                 # main effects of d = 4 take 3 columns
    with pytest.raises(ValueError, match="^Xint.*contiguous"):
        mr(X, al, beta, s, [0], t, Xint=torch.zeros((3, 20), dtype=f64).t())
    with pytest.raises(ValueError, match="^Xint.*exceed"):
        mr(X, al, beta, s, [0], t, Xint=torch.zeros((700, 3), dtype=f64))
    with pytest.raises(ValueError, match="^Xint.*nothing"):
        mr(X[:, :1].contiguous(), al, beta[:, :1].contiguous(), s, [0], t,
           Xint=torch.zeros((3, 1), dtype=f64))
    with pytest.raises(ValueError, match="^out"):
        mr(X, al, beta, s, [0, 1], t, Xint=Xm, out=torch.zeros((2, 2, 12), dtype=f64))
    with pytest.raises(ValueError, match="^out"):
        mr(X, al, beta, s, [(0, 1)], t, t, Xint=Xp, out=torch.zeros((2, 1, 121), dtype=f64))
    with pytest.raises(ValueError, match="HIP device"):
        mr(X, al, beta, s, [0, 3], t, Xint=Xm)              # all valid, but on the host
    with pytest.raises(ValueError, match="HIP device"):
        mr(X, al, beta, s, [(3, 0)], t, t, Xint=Xp)

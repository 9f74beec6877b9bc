"""CPU: gp_sobol_exact / gp_sobol_exact_ws_bytes are declared, exported and bound, every argument
check answers on the host (minus the argument's position) before any launch, and
kernels.sobol_exact validates dtype, shape, contiguity, grouping, the box and the device before
the call.

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
NAMES = ("gp_sobol_exact", "gp_sobol_exact_ws_bytes")


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
    assert len(_capi.SIGNATURES["gp_sobol_exact"][1]) == 22
    assert len(_capi.SIGNATURES["gp_sobol_exact_ws_bytes"][1]) == 4
    decl = re.search(r"int gp_sobol_exact\((.*?)\);", src, flags=re.S).group(1)
    assert len(decl.split(",")) == 22
    assert "sobolx.hip" in _build.SOURCES


(X, N, D, LDX, G, M, ALPHA, LDA, BETA, LDBETA, S, LO, HI, E, INCE, Q, LDQ, LDQA, LDQG, WS, WSB,
 STREAM) = range(1, 23)
_P = ctypes.c_void_p(256)


def _args(**over):
    """A valid call -- n = 100, d = 8, two groups of three units, tight strides -- up to its null
    workspace (so it returns -WS and nothing is launched)."""
    a = {X: _P, N: 100, D: 8, LDX: 8, G: 2, M: 3, ALPHA: _P, LDA: 100, BETA: _P, LDBETA: 8, S: _P,
         LO: None, HI: None, E: _P, INCE: 1, Q: _P, LDQ: 17, LDQA: 51, LDQG: 153, WS: None,
         WSB: 1 << 40, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 23)]


@pytest.mark.parametrize("over,code", [
    (dict(), -WS),                                          # valid up to the null workspace
    (dict(X=None), -X),
    (dict(N=-1), -N),
    (dict(D=0), -D), (dict(D=33, LDX=33, LDBETA=33, LDQ=67, LDQA=201, LDQG=603), -D),
    (dict(D=32, LDX=32, LDBETA=32, LDQ=65, LDQA=195, LDQG=585), -WS),
    (dict(LDX=7), -LDX),
    (dict(G=-1), -G),
    (dict(M=0), -M), (dict(M=-2), -M),
    (dict(G=1 << 20, M=1 << 20), -M),                       # G M beyond an int
    (dict(ALPHA=None), -ALPHA),
    (dict(LDA=99), -LDA),
    (dict(LDA=0, G=1, M=1), -WS),                           # one unit: no unit strides
    (dict(BETA=None), -BETA),
    (dict(LDBETA=7), -LDBETA),
    (dict(LDBETA=0, INCE=0, G=1, M=1), -WS),
    (dict(S=None), -S),
    (dict(LO=_P), -HI), (dict(HI=_P), -LO),                 # both bounds or neither
    (dict(LO=_P, HI=_P), -WS),
    (dict(E=None), -E),
    (dict(INCE=0), -INCE),
    (dict(INCE=5), -WS),
    (dict(Q=None), -Q),
    (dict(LDQ=16), -LDQ),
    (dict(LDQ=16, LDQA=0, LDQG=17, M=1), -WS),              # M = 1: ldq, ldqa are not strides
    (dict(LDQA=50), -LDQA),
    (dict(LDQ=20, LDQA=56), -LDQA),                         # (M - 1) ldq + 2 d + 1 = 57
    (dict(LDQ=20, LDQA=57, LDQG=2 * 77 + 17), -WS),
    (dict(LDQG=152), -LDQG),
    (dict(LDQG=0, G=1), -WS),                               # one group: no group stride
    (dict(LDQG=16, M=1), -LDQG), (dict(LDQG=17, M=1), -WS),
    (dict(WS=ctypes.c_void_p(16)), -WS),                    # workspace not 256-B aligned
    (dict(WS=_P, WSB=16), -WSB),
    (dict(G=0), 0), (dict(G=0, WS=None, WSB=0), 0),         # no groups: validated, no launch
    (dict(G=0, Q=None), -Q),                                # ... after the checks
    # two faults: the earlier argument is reported
    (dict(X=None, N=-1), -X), (dict(N=-1, D=0), -N), (dict(LDX=7, G=-1), -LDX),
    (dict(M=0, ALPHA=None), -M), (dict(LDA=99, BETA=None), -LDA), (dict(S=None, E=None), -S),
    (dict(INCE=0, Q=None), -INCE), (dict(LDQ=16, LDQG=0), -LDQ),
    (dict(LDQG=0, WS=_P, WSB=0), -LDQG),
])
def test_argument_checks(lib, over, code):
    assert lib.gp_sobol_exact(*_args(**over)) == code


def test_workspace_size(lib):
    f = lib.gp_sobol_exact_ws_bytes
    one = f(512, 8, 1, 1)
    # the one-point integrals and their leave-one-out products, and 2 d + 1 sums per tile
    assert one >= 8 * (2 * 512 * 8 + 17 * 64) and one % 256 == 0
    sizes = [f(n, 8, 2, 3) for n in (1, 17, 64, 65, 128, 129, 512, 513, 2000)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    sizes = [f(300, d, 2, 3) for d in (1, 2, 8, 9, 32)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    sizes = [f(300, 8, g, 3) for g in (1, 2, 64, 1000)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    sizes = [f(300, 8, 2, m) for m in (1, 2, 5, 32)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert f(512, 8, 8, 32) < 1 << 30                       # the reference configuration
    assert f(0, 8, 2, 3) == 0 and f(512, 8, 0, 3) == 0
    for bad in ((-1, 8, 1, 1), (512, -1, 1, 1), (512, 8, -1, 1), (512, 8, 1, -1)):
        assert f(*bad) == -1, bad
    # one byte less than the exact size is refused (the exact size would launch: a GPU test's)
    assert lib.gp_sobol_exact(*_args(WS=_P, WSB=f(100, 8, 2, 3) - 1)) == -WSB


def test_sobol_exact_validates_before_the_call():
    """Every ValueError names its argument; nothing reaches the library (the operands are host
    tensors, which the last check refuses too)."""
    from gladsgp_amd import kernels
    f64 = torch.float64
    X = torch.zeros((10, 4), dtype=f64)
    al = torch.zeros((6, 10), dtype=f64)
    beta = torch.ones((6, 4), dtype=f64)
    s = torch.ones(6, dtype=f64)
    lo, hi = torch.zeros(4, dtype=f64), torch.ones(4, dtype=f64)
    sx = kernels.sobol_exact
    with pytest.raises(ValueError, match="^X"):
        sx(X.float(), al, beta, s)
    with pytest.raises(ValueError, match="^X.*contiguous"):
        sx(torch.zeros((4, 10), dtype=f64).t(), al, beta, s)
    with pytest.raises(ValueError, match="^X.*GPFIT_MAX_DIM"):
        sx(torch.zeros((10, 33), dtype=f64), al, torch.ones((6, 33), dtype=f64), s)
    with pytest.raises(ValueError, match="^alpha.*shape"):
        sx(X, torch.zeros((6, 9), dtype=f64), beta, s)
    with pytest.raises(ValueError, match="^alpha"):
        sx(X, al.float(), beta, s)
    with pytest.raises(ValueError, match="^alpha.*contiguous"):
        sx(X, torch.zeros((10, 6), dtype=f64).t(), beta, s)
    with pytest.raises(ValueError, match="^beta.*shape"):
        sx(X, al, torch.ones((6, 3), dtype=f64), s)
    with pytest.raises(ValueError, match="^beta.*contiguous"):
        sx(X, al, torch.ones((4, 6), dtype=f64).t(), s)
    with pytest.raises(ValueError, match="^s:"):
        sx(X, al, beta, torch.ones(5, dtype=f64))
    with pytest.raises(ValueError, match="^group"):
        sx(X, al, beta, s, group=0)
    with pytest.raises(ValueError, match="^group"):
        sx(X, al, beta, s, group=2.0)
    with pytest.raises(ValueError, match="^group.*whole"):
        sx(X, al, beta, s, group=4)
    with pytest.raises(ValueError, match="^lo, hi.*both"):
        sx(X, al, beta, s, lo=lo)
    with pytest.raises(ValueError, match="^lo, hi.*both"):
        sx(X, al, beta, s, hi=hi)
    with pytest.raises(ValueError, match="^lo.*shape"):
        sx(X, al, beta, s, lo=torch.zeros(3, dtype=f64), hi=hi)
    with pytest.raises(ValueError, match="^hi"):
        sx(X, al, beta, s, lo=lo, hi=hi.float())
    with pytest.raises(ValueError, match="^out"):
        sx(X, al, beta, s, group=3, out=(torch.zeros(6, dtype=f64),
                                         torch.zeros((2, 3, 3, 8), dtype=f64)))
    with pytest.raises(ValueError, match="^out"):
        sx(X, al, beta, s, group=3, out=torch.zeros(6, dtype=f64))
    with pytest.raises(ValueError, match="^out"):
        sx(X, al, beta, s, out=(torch.zeros(6, dtype=torch.float32),
                                torch.zeros((6, 1, 1, 9), dtype=f64)))
    with pytest.raises(ValueError, match="HIP device"):
        sx(X, al, beta, s, group=3)                         # all valid, but on the host
    with pytest.raises(ValueError, match="HIP device"):
        sx(X, al, beta, s, lo=lo, hi=hi)


def test_box_order_is_checked_before_the_call(monkeypatch):
    """hi <= lo in any dimension is refused by the Python layer (the C call cannot see it without
    a synchronisation and documents the result as unspecified)."""
    from gladsgp_amd import kernels
    monkeypatch.setattr(kernels, "_check_device", lambda t, name: None)
    f64 = torch.float64
    X = torch.zeros((10, 2), dtype=f64)
    al, beta = torch.zeros((1, 10), dtype=f64), torch.ones((1, 2), dtype=f64)
    s = torch.ones(1, dtype=f64)
    for lo, hi in (([0.0, 0.5], [1.0, 0.5]), ([0.0, 0.6], [1.0, 0.5])):
        with pytest.raises(ValueError, match="^lo, hi.*exceed"):
            kernels.sobol_exact(X, al, beta, s, lo=torch.tensor(lo, dtype=f64),
                                hi=torch.tensor(hi, dtype=f64))


def test_public_surface_validates():
    from gladsgp_amd import sensitivity
    with pytest.raises(ValueError, match="EmulatorModel"):
        sensitivity.exact_indices(object(), {})
    r = sensitivity.ExactSobolResult(torch.zeros((2, 3)), torch.ones((2, 3)), None, None,
                                     torch.zeros(2), torch.ones(2), "mean")
    assert torch.equal(r.interaction, torch.ones((2, 3)))
    with pytest.raises(ValueError, match="^interval"):
        r.interval()
    h = r.numpy()
    assert h.first_order.shape == (2, 3) and h.general_first_order is None and h.average == "mean"

"""CPU: gp_field / gp_field_max_pcs are declared, exported and bound, and every argument check of
gp_field answers on the host (LAPACK-style negative argument number) before any launch.

No device work happens here: the pointers handed over are never dereferenced.
"""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpfit.h")
NAMES = ("gp_field", "gp_field_max_pcs")


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
    assert len(_capi.SIGNATURES["gp_field"][1]) == 14
    assert "field.hip" in _build.SOURCES


def test_max_pcs_is_sixty_four(lib):
    from gladsgp_amd import blas
    assert lib.gp_field_max_pcs() == 64
    assert blas.field_max_pcs() == 64


# argument positions (1-based, the code returned is their negative)
W, LDW, ROWS, P, K, LDK, NCOLS, SD, MU, ERR, Y, LDY, F32, STREAM = range(1, 15)


def _args(**over):
    d = ctypes.c_void_p(64)
    a = {W: d, LDW: 8, ROWS: 40, P: 8, K: d, LDK: 100, NCOLS: 100, SD: None, MU: None, ERR: None,
         Y: d, LDY: 100, F32: 0, STREAM: None}
    for k, v in over.items():
        a[globals()[k]] = v
    return [a[i] for i in range(1, 15)]


@pytest.mark.parametrize("over,code", [
    (dict(W=None), -W),
    (dict(LDW=7), -LDW),                       # ldw < P
    (dict(LDW=0, P=0), -LDW),                  # ldw < 1 (before P is looked at)
    (dict(ROWS=-1), -ROWS),
    (dict(P=0), -P),
    (dict(P=65, LDW=65), -P),                  # P > gp_field_max_pcs()
    (dict(K=None), -K),
    (dict(LDK=99), -LDK),                      # ldk < ncols
    (dict(LDK=0, NCOLS=0), -LDK),              # ldk < 1 (before ncols is looked at)
    (dict(NCOLS=-1), -NCOLS),
    (dict(SD=ctypes.c_void_p(64)), -SD),       # sd without mu
    (dict(MU=ctypes.c_void_p(64)), -SD),       # mu without sd
    (dict(Y=None), -Y),
    (dict(LDY=99), -LDY),                      # ldy < ncols
    (dict(LDY=0, NCOLS=0), -LDY),              # ldy < 1
    (dict(Y=None, F32=1), -Y),                 # the same checks for the float32 output
    (dict(LDY=99, F32=1), -LDY),
])
def test_argument_checks(lib, over, code):
    assert lib.gp_field(*_args(**over)) == code


def test_first_wrong_argument_wins(lib):
    assert lib.gp_field(*_args(W=None, Y=None)) == -W
    assert lib.gp_field(*_args(P=65, LDW=65, Y=None)) == -P
    assert lib.gp_field(*_args(ROWS=0, Y=None)) == -Y          # checked before the empty return


@pytest.mark.parametrize("f32", [0, 1])
def test_empty_problem_is_a_no_op(lib, f32):
    """rows = 0 or ncols = 0 on otherwise valid arguments returns 0 before any launch."""
    assert lib.gp_field(*_args(ROWS=0, F32=f32)) == 0
    assert lib.gp_field(*_args(NCOLS=0, F32=f32)) == 0
    assert lib.gp_field(*_args(ROWS=0, NCOLS=0, P=64, LDW=64, F32=f32)) == 0

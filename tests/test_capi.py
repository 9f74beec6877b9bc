"""CPU: the C-ABI library builds, loads, and exports every symbol include/gpfit.h declares.

No device work happens here: only host-side entry points (sizes, argument validation that
returns before any launch) are called.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpfit.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gp_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from gladsgp_amd import _build, _capi
    _build.build_library()
    return _capi.lib()


def test_header_declares_expected_entry_points():
    names = _declared()
    for must in ("gp_gram_ardse", "gp_cross_ardse", "gp_potrf_inv", "gp_predict",
                 "gp_predict_ws_bytes", "gp_nll", "gp_trmv", "gp_padded_n", "gp_version",
                 "gp_loglik", "gp_loglik_ws_bytes"):
        assert must in names


def test_every_declared_symbol_is_exported(lib):
    from gladsgp_amd import _build, _capi
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gp_[a-z_0-9]+)", out))
    for name in _declared():
        assert name in exported, name
        assert name in _capi.SIGNATURES, f"{name} lacks a ctypes signature"
    # _capi.lib() binds what it finds (older builds in same-box A/B runs): the shipped build
    # must export every signature it knows
    for name in _capi.SIGNATURES:
        assert name in exported, name
        assert getattr(lib, name).argtypes is not None or not _capi.SIGNATURES[name][1], name


def test_library_has_gfx950_code_object():
    from gladsgp_amd import _build
    data = open(_build.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data


def test_host_side_helpers(lib):
    assert lib.gp_version() >= 100
    assert lib.gp_padded_n(1) == 128
    assert lib.gp_padded_n(4096) == 4096
    assert lib.gp_padded_n(4097) == 4224
    assert lib.gp_padded_n(0) == 0
    ws = lib.gp_predict_ws_bytes(4096, 100000, 1, 0)
    assert ws > 4096 * 4096 * 8 // 4
    # a given chunk bounds the cross-covariance scratch
    small = lib.gp_predict_ws_bytes(4096, 100000, 1, 1024)
    assert small < ws
    assert lib.gp_predict_ws_bytes(0, 10, 1, 0) == 0


def test_argument_validation_returns_lapack_style_codes(lib):
    # invalid arguments are rejected on the host before any launch
    rc = lib.gp_gram_ardse(None, 10, 2, 2, None, 2, None, None, None, 10, 100, 1, None)
    assert rc == -1
    dummy = ctypes.c_void_p(16)
    rc = lib.gp_gram_ardse(dummy, 10, 0, 2, dummy, 2, dummy, dummy, dummy, 10, 100, 1, None)
    assert rc == -3   # d out of range
    rc = lib.gp_gram_ardse(dummy, 10, 2, 2, dummy, 2, dummy, dummy, dummy, 5, 100, 1, None)
    assert rc == -10  # ldg < n
    rc = lib.gp_potrf_inv(dummy, 100, 100, 10000, dummy, 64, 4096, 1, None, None, None)
    assert rc == -6   # ldinv < gp_padded_n(n)
    rc = lib.gp_predict(dummy, 128, 128 * 128, dummy, 2, dummy, 2, 100, 10, 2, dummy, 2, dummy,
                        dummy, dummy, 100, dummy, dummy, 10, 1, dummy, 0, 0, None)
    assert rc == -22  # workspace too small
    # zero-sized problems are a no-op
    assert lib.gp_potrf_inv(dummy, 0, 1, 0, dummy, 1, 0, 1, None, None, None) == 0
    # gp_loglik: workspace size grows with the batch; bad args rejected before any launch
    assert lib.gp_loglik_ws_bytes(512, 8) > lib.gp_loglik_ws_bytes(512, 1) > 512 * 512 * 8
    assert lib.gp_loglik_ws_bytes(-1, 1) == -1
    rc = lib.gp_loglik(dummy, 64, 0, 2, dummy, 2, dummy, dummy, dummy, 64, 1, dummy, 1 << 30,
                       dummy, None, None)
    assert rc == -3   # d < 1
    wsp = ctypes.c_void_p(256)                       # workspaces are 256-B aligned
    rc = lib.gp_loglik(dummy, 64, 2, 2, dummy, 2, dummy, dummy, dummy, 64, 2, wsp, 16,
                       dummy, None, None)
    assert rc == -13  # workspace too small
    rc = lib.gp_loglik(dummy, 64, 2, 2, dummy, 2, dummy, dummy, dummy, 64, 2, dummy, 1 << 30,
                       dummy, None, None)
    assert rc == -12  # workspace not 256-B aligned
    assert lib.gp_loglik(dummy, 0, 2, 2, dummy, 2, dummy, dummy, dummy, 0, 1, None, 0, dummy,
                         None, None) == 0
    # gp_fit_predict: validated before anything is enqueued
    assert lib.gp_fit_predict_ws_bytes(4096, 100000, 1, 0) >= lib.gp_predict_ws_bytes(4096,
                                                                                       100000,
                                                                                       1, 0)
    args = [dummy, 2, dummy, 2, 100, 10, 2, dummy, 2, dummy, dummy, dummy, dummy, 100,
            dummy, 100, 10000, dummy, 128, 128 * 128, None, None, dummy, dummy, 10, 1, wsp,
            1 << 40, 0, None, None]
    bad = list(args)
    bad[10] = None                                   # delta
    assert lib.gp_fit_predict(*bad) == -24
    bad = list(args)
    bad[15] = 50                                     # ldg < n
    assert lib.gp_fit_predict(*bad) == -26
    bad = list(args)
    bad[27] = 16                                     # workspace too small
    assert lib.gp_fit_predict(*bad) == -22
    bad[26] = ctypes.c_void_p(16)                    # workspace not 256-B aligned
    bad[27] = 1 << 40
    assert lib.gp_fit_predict(*bad) == -21


def test_new_entry_points_validate(lib):
    """gp_potrf / gp_trtri / gp_predict_chol / gp_ctx_*: argument checks before any launch."""
    dummy = ctypes.c_void_p(16)
    assert lib.gp_potrf(None, 4, 4, 16, 1, None, None, None) == -1
    assert lib.gp_potrf(dummy, 4, 3, 16, 1, None, None, None) == -3
    assert lib.gp_potrf(dummy, 4, 4, 8, 2, None, None, None) == -4
    assert lib.gp_potrf(dummy, 0, 1, 0, 1, None, None, None) == 0
    assert lib.gp_trtri(None, 4, 4, 16, dummy, 128, 128 * 128, 1, None, None) == -1
    assert lib.gp_trtri(dummy, 4, 4, 16, dummy, 64, 128 * 128, 1, None, None) == -6
    assert lib.gp_trtri(dummy, 4, 4, 16, None, 128, 128 * 128, 1, None, None) == -5
    assert lib.gp_predict_chol_ws_bytes(4096, 100000, 1, 0) == (
        8 * 4096 * 4096 + lib.gp_predict_ws_bytes(4096, 100000, 1, 0))
    args = [dummy, 100, 10000, dummy, 2, dummy, 2, 100, 10, 2, dummy, 2, dummy, dummy, dummy,
            100, dummy, dummy, 10, 1, None, dummy, 1 << 40, 0, None]
    bad = list(args)
    bad[0] = None
    assert lib.gp_predict_chol(*bad) == -1
    bad = list(args)
    bad[22] = 16                                     # workspace too small
    assert lib.gp_predict_chol(*bad) == -23
    assert lib.gp_ctx_create(2.0, 0, dummy) == -1
    assert lib.gp_ctx_create(0.4, 0, None) == -3
    assert lib.gp_ctx_destroy(None) == 0
    assert lib.gp_ctx_set_aux_chunks(None, 1) == -1
    assert lib.gp_ctx_set_aux_chunks(dummy, -5) == -2      # rejected before the handle is read


# Return codes of the prediction entry points.  Each base argument list is valid except for a
# null workspace, so the call returns that code and never reaches a launch; every row breaks
# the named arguments of the base list and gives the code the library must return.  Rows with
# two faults pin the order in which errors are reported.
_P = 16          # a non-null, 16-B aligned address (never dereferenced)
_N, _M, _NPAD = 100, 10, 128
_CROSS = dict(X=_P, ldx=2, Xs=_P, ldxs=2, n=_N, m=_M, d=2, beta=_P, ldbeta=2, s=_P)
_LINV = dict(Linv=_P, ldinv=_NPAD, strideInv=_NPAD * _NPAD)
_OUT = dict(s_pred=_P, w_hat=_P, ldw=_N, mean=_P, var=_P, ldo=_M)
_WS = dict(batch=2, ws=None, ws_bytes=1 << 40, m_chunk=0)
_PACKED_ELEMS = _NPAD * _NPAD - 128 * 8 * 7      # gp_linv_packed_elems(100)


def _rows_cross(c):
    """check_common's codes; c maps the shared names to this entry point's codes."""
    return [(dict(X=None), c["X"]), (dict(ldx=1), c["ldx"]), (dict(Xs=None), c["Xs"]),
            (dict(ldxs=1), c["ldxs"]), (dict(n=-1), c["n"]), (dict(m=-1), c["m"]),
            (dict(d=0), c["d"]), (dict(d=33, ldx=33, ldxs=33, ldbeta=33), c["d"]),
            (dict(beta=None), c["beta"]), (dict(ldbeta=1), c["ldbeta"]),
            (dict(ldbeta=1, batch=1), c["ws"]),             # ldbeta is a batch stride
            (dict(s=None), c["s"]), (dict(batch=-1), c["batch"]),
            (dict(X=None, ldx=1), c["X"]), (dict(s=None, batch=-1), c["s"]),
            (dict(n=0), 0), (dict(m=0), 0), (dict(batch=0), 0)]


def _rows_linv(c):
    """The L^-1 pointer / leading dimension / stride codes (padded layout)."""
    return [(dict(Linv=None), c["Linv"]), (dict(Linv=8), c["Linv"]),
            (dict(ldinv=64), c["ldinv"]), (dict(ldinv=_NPAD + 1), c["ldinv"]),
            (dict(strideInv=_NPAD * _NPAD - 2), c["strideInv"]),
            (dict(strideInv=_NPAD * _NPAD + 1), c["strideInv"]),
            (dict(strideInv=0, batch=1), c["ws"]),          # one problem: no stride to check
            (dict(strideInv=1, batch=1), c["strideInv"]),   # ... but it must stay even
            (dict(Linv=None, ldinv=64), c["Linv"]),
            (dict(ldinv=64, strideInv=1), c["ldinv"])]


def _rows_out(c):
    return [(dict(s_pred=None), c["s_pred"]), (dict(w_hat=None), c["w_hat"]),
            (dict(ldw=_N - 1), c["ldw"]), (dict(ldw=0, batch=1), c["ws"]),
            (dict(mean=None), c["mean"]), (dict(var=None), c["var"]),
            (dict(ldo=_M - 1), c["ldo"]), (dict(ldo=0, batch=1), c["ws"]),
            (dict(s_pred=None, var=None), c["s_pred"]), (dict(mean=None, ldo=0), c["mean"])]


_SOLVE_CODES = dict(Linv=-1, ldinv=-2, strideInv=-3, s_pred=-14, w_hat=-15, ldw=-16, mean=-17,
                    var=-18, ldo=-19)
_COMMON_CODES = dict(X=-4, ldx=-5, Xs=-6, ldxs=-7, n=-8, m=-9, d=-10, beta=-11, ldbeta=-12,
                     s=-13, batch=-20)


def _predict_ex_table():
    c = dict(_COMMON_CODES, **_SOLVE_CODES, ws=-21)
    order = ["Linv", "ldinv", "strideInv", "X", "ldx", "Xs", "ldxs", "n", "m", "d", "beta",
             "ldbeta", "s", "s_pred", "w_hat", "ldw", "mean", "var", "ldo", "batch", "ws",
             "ws_bytes", "m_chunk", "layout", "z", "ldz", "stream"]
    base = dict(_LINV, **_CROSS, **_OUT, **_WS, layout=0, z=None, ldz=0, stream=None)
    rows = _rows_cross(c) + _rows_linv(c) + _rows_out(c) + [
        (dict(layout=2), -24), (dict(layout=-1), -24),
        (dict(layout=2, Linv=None), -24),                   # layout before L^-1
        (dict(layout=2, X=None), -24),
        (dict(Linv=None, X=None), -4),                      # the design before L^-1
        (dict(X=None, mean=None), -4),
        (dict(layout=1, ldinv=0), -21),                     # packed: ldinv ignored
        (dict(layout=1, strideInv=_PACKED_ELEMS), -21),
        (dict(layout=1, strideInv=_PACKED_ELEMS - 2), -3),
        (dict(layout=1, Linv=8), -1),
        (dict(z=_P, ldz=_NPAD), -21),
        (dict(z=_P, ldz=_NPAD, w_hat=None), -21),           # with z, w_hat is not read
        (dict(z=_P, ldz=_NPAD - 1), -26),
        (dict(z=_P, ldz=0, batch=1), -21),
        (dict(z=_P, ldz=_NPAD - 1, mean=None), -17),        # outputs before ldz
        (dict(z=_P, ldz=-1, n=0), -26),                     # ... and ldz before the no-op
        (dict(n=0, ldinv=0), -2), (dict(n=0, ldinv=2, strideInv=0), 0),
        (dict(m_chunk=-1), -23),                            # m_chunk before the workspace
        (dict(m_chunk=-1, n=0), 0),                         # ... and after the no-op
        (dict(m_chunk=-1, ldo=0), -19),
        (dict(ws=16), -21),                                 # workspace not 256-B aligned
        (dict(ws=256, ws_bytes=16), -22), (dict(ws=256, ws_bytes=16, m_chunk=-1), -23)]
    return "gp_predict_ex", order, base, -21, rows


def _predict_cross_table():
    c = dict(_COMMON_CODES, ws=-21)
    order = ["X", "ldx", "Xs", "ldxs", "n", "m", "d", "beta", "ldbeta", "s", "batch", "ws",
             "ws_bytes", "m_chunk", "stream"]
    base = dict(_CROSS, **_WS, stream=None)
    rows = _rows_cross(c) + [
        (dict(m_chunk=-1), -23), (dict(m_chunk=-1, m=0), 0), (dict(m_chunk=-1, s=None), -13),
        (dict(ws=16), -21),
        (dict(ws=256, ws_bytes=16), -22), (dict(ws=256, ws_bytes=16, m_chunk=-1), -23)]
    return "gp_predict_cross", order, base, -21, rows


def _predict_solve_table():
    c = dict(_SOLVE_CODES, ws=-21)
    order = ["Linv", "ldinv", "strideInv", "n", "m", "s_pred", "w_hat", "ldw", "mean", "var",
             "ldo", "batch", "ws", "ws_bytes", "m_chunk", "stream"]
    base = dict(_LINV, n=_N, m=_M, **_OUT, **_WS, stream=None)
    rows = _rows_linv(c) + _rows_out(c) + [
        (dict(n=-1), -4), (dict(m=-1), -5), (dict(batch=-1), -12),
        (dict(n=-1, Linv=None), -4), (dict(batch=-1, Linv=None), -12),   # sizes before L^-1
        (dict(n=-1, m=-1), -4), (dict(m=-1, batch=-1), -5),
        (dict(n=0), 0), (dict(m=0), 0), (dict(batch=0), 0),
        (dict(n=0, ldinv=0), -2), (dict(n=0, mean=None), -17),
        (dict(m_chunk=-1), -23), (dict(m_chunk=-1, m=0), 0), (dict(m_chunk=-1, var=None), -18),
        (dict(ws=16), -21),
        (dict(ws=256, ws_bytes=16), -22), (dict(ws=256, ws_bytes=16, m_chunk=-1), -23)]
    return "gp_predict_solve", order, base, -21, rows


def _predict_z_table():
    order = ["Linv", "ldinv", "strideInv", "layout", "n", "w_hat", "ldw", "z", "ldz", "batch",
             "ws", "ws_bytes", "stream"]
    base = dict(_LINV, layout=0, n=_N, w_hat=_P, ldw=_N, z=_P, ldz=_NPAD, batch=2, ws=None,
                ws_bytes=1 << 40, stream=None)
    c = dict(Linv=-1, ldinv=-2, strideInv=-3, ws=-11)
    rows = _rows_linv(c) + [
        (dict(layout=2), -4), (dict(n=-1), -5), (dict(w_hat=None), -6), (dict(ldw=_N - 1), -7),
        (dict(ldw=0, batch=1), -11), (dict(z=None), -8), (dict(ldz=_NPAD - 1), -9),
        (dict(ldz=0, batch=1), -11), (dict(batch=-1), -10),
        (dict(Linv=None, layout=2), -1),                    # L^-1's pointer before the layout
        (dict(Linv=8, n=-1), -1),
        (dict(layout=2, ldinv=64), -4), (dict(layout=2, n=-1), -4),
        (dict(n=-1, ldinv=-1), -5), (dict(n=-1, strideInv=1), -5),   # n before ld / stride
        (dict(ldinv=64, w_hat=None), -2), (dict(strideInv=1, w_hat=None), -3),
        (dict(w_hat=None, z=None), -6), (dict(z=None, batch=-1), -8),
        (dict(layout=1, ldinv=0), -11), (dict(layout=1, strideInv=_PACKED_ELEMS), -11),
        (dict(layout=1, strideInv=_PACKED_ELEMS - 2), -3),
        (dict(n=0), 0), (dict(batch=0), 0), (dict(n=0, ldinv=0), 0),
        (dict(n=0, batch=-1), -10),
        (dict(ws=16), -11), (dict(ws=256, ws_bytes=16), -12)]
    return "gp_predict_z", order, base, -11, rows


def _predict_chol_table():
    c = dict(_COMMON_CODES, ws=-22)
    order = ["L", "ldl", "strideL", "X", "ldx", "Xs", "ldxs", "n", "m", "d", "beta", "ldbeta",
             "s", "s_pred", "w_hat", "ldw", "mean", "var", "ldo", "batch", "info", "ws",
             "ws_bytes", "m_chunk", "stream"]
    base = dict(L=_P, ldl=_N, strideL=_N * _N, **_CROSS, **_OUT, **_WS, info=None, stream=None)
    rows = _rows_cross(c) + [
        (dict(L=None), -1), (dict(ldl=_N - 1), -2), (dict(strideL=_N * _N - 1), -3),
        (dict(strideL=0, batch=1), -22),
        (dict(L=None, X=None), -1), (dict(ldl=_N - 1, X=None), -2), (dict(strideL=0, X=None), -3),
        (dict(m_chunk=-1), -24),                            # m_chunk before the workspace
        (dict(m_chunk=-1, n=0), 0),
        (dict(ws=16), -22),
        (dict(ws=256, ws_bytes=16), -23), (dict(ws=256, ws_bytes=16, m_chunk=-1), -24)]
    return "gp_predict_chol", order, base, -22, rows


def _fit_predict_table():
    c = dict(_COMMON_CODES, **_SOLVE_CODES, ws=-21)
    order = ["X", "ldx", "Xs", "ldxs", "n", "m", "d", "beta", "ldbeta", "s", "delta", "s_pred",
             "w_hat", "ldw", "G", "ldg", "strideG", "Linv", "ldinv", "strideInv", "info",
             "logdet", "mean", "var", "ldo", "batch", "ws", "ws_bytes", "m_chunk", "ctx",
             "stream"]
    base = dict(_CROSS, **_LINV, **_OUT, **_WS, delta=_P, G=_P, ldg=_N, strideG=_N * _N,
                info=None, logdet=None, ctx=None, stream=None)
    rows = _rows_cross(c) + _rows_linv(c) + _rows_out(c) + [
        (dict(delta=None), -24), (dict(G=None), -25), (dict(ldg=_N - 1), -26),
        (dict(strideG=_N * _N - 1), -26), (dict(strideG=0, batch=1), -21),
        (dict(Linv=None, X=None), -4), (dict(delta=None, ldo=0), -19),
        (dict(delta=None, G=None), -24), (dict(G=None, n=0), -25),
        (dict(m_chunk=-1), -23), (dict(m_chunk=-1, n=0), 0), (dict(m_chunk=-1, ldg=0), -26),
        (dict(ws=16), -21),                                 # workspace not 256-B aligned
        (dict(ws=256, ws_bytes=16), -22), (dict(ws=16, ws_bytes=16), -21),
        (dict(ws=256, ws_bytes=16, m_chunk=-1), -23)]
    return "gp_fit_predict", order, base, -21, rows


@pytest.mark.parametrize("table", [_predict_ex_table, _predict_cross_table,
                                   _predict_solve_table, _predict_z_table,
                                   _predict_chol_table, _fit_predict_table],
                         ids=lambda t: t.__name__.strip("_"))
def test_prediction_return_codes(lib, table):
    """gp_predict_ex / _cross / _solve / _z / _chol and gp_fit_predict: which argument is
    reported, and in which order, before anything is enqueued."""
    name, order, base, base_rc, rows = table()
    assert sorted(order) == sorted(base), name
    fn = getattr(lib, name)
    assert fn(*[base[k] for k in order]) == base_rc
    got = []
    for change, _ in rows:
        assert set(change) <= set(base), (name, change)
        got.append(fn(*[dict(base, **change)[k] for k in order]))
    assert got == [rc for _, rc in rows], [
        (change, want, g) for (change, want), g in zip(rows, got) if g != want]


# Return codes of the factorisation entry points, in the same form.  No row may reach an
# allocation or a launch (the pointers are dummies): the bases of the allocating forms and of
# gp_trtri have n = 0 (a valid no-op, where one changed field still reaches every code), those
# of the _ws forms a workspace that is too small.  Rows change one field; the few with two
# faults pin the order of the checks.
_FACT = dict(A=_P, n=0, lda=1, strideA=0, batch=2, info=None, stream=None)
_FACT_INV = dict(_FACT, Linv=_P, ldinv=1, strideInv=0)
_FACT_N = dict(n=_N, lda=_N, strideA=_N * _N)
_INV_ORDER = ["A", "n", "lda", "strideA", "Linv", "ldinv", "strideInv", "batch", "info"]


def _rows_fact(batch_rc):
    """potrf_args' codes (the plain forms), shared by the inverse forms up to the batch."""
    return [(dict(A=None), -1), (dict(n=-1), -2), (dict(lda=0), -3), (dict(strideA=-1), -4),
            (dict(batch=-1), batch_rc), (dict(batch=0), 0),
            (dict(strideA=-1, batch=1), 0),                 # one problem: no stride to check
            (dict(A=None, n=-1), -1), (dict(n=-1, lda=0), -2), (dict(lda=0, strideA=-1), -3)]


def _rows_fact_inv():
    return _rows_fact(-8) + [
        (dict(Linv=None), -5), (dict(ldinv=0), -6), (dict(strideInv=-1), -7),
        (dict(strideInv=-1, batch=1), 0),
        (dict(strideA=-1, Linv=None), -4), (dict(Linv=None, ldinv=0), -5),
        (dict(ldinv=0, strideInv=-1), -6), (dict(ldinv=0, batch=-1), -6)]


# the same codes at n > 0 (every row still fails validation)
_ROWS_FACT_N = [(dict(A=None), -1), (dict(n=-1), -2), (dict(lda=_N - 1), -3),
                (dict(strideA=_N * _N - 1), -4)]
_ROWS_FACT_INV_N = _ROWS_FACT_N + [
    (dict(Linv=None), -5), (dict(ldinv=_NPAD - 1), -6), (dict(ldinv=64), -6),
    (dict(strideInv=_NPAD * _NPAD - 1), -7), (dict(batch=-1), -8), (dict(batch=0), 0),
    (dict(n=0), 0)]


def _potrf_inv_table():
    order = _INV_ORDER + ["logdet", "stream"]
    return "gp_potrf_inv", order, dict(_FACT_INV, logdet=None), 0, _rows_fact_inv()


def _potrf_inv_ws_table():
    order = _INV_ORDER + ["logdet", "ws", "ws_bytes", "stream"]
    base = dict(_FACT_INV, **_FACT_N, ldinv=_NPAD, strideInv=_NPAD * _NPAD, logdet=None,
                ws=256, ws_bytes=16)
    rows = _ROWS_FACT_INV_N + [
        (dict(ws=None), -11), (dict(ws=16), -11),           # workspace not 256-B aligned
        (dict(ws=None, ws_bytes=1 << 40), -11), (dict(ws=None, Linv=None), -5),
        (dict(ws_bytes=0), -12), (dict(ws_bytes=16, batch=-1), -8)]
    return "gp_potrf_inv_ws", order, base, -12, rows


def _potrf_table():
    order = ["A", "n", "lda", "strideA", "batch", "info", "logdet", "stream"]
    return "gp_potrf", order, dict(_FACT, logdet=None), 0, _rows_fact(-5)


def _potrf_ws_table():
    order = ["A", "n", "lda", "strideA", "batch", "info", "logdet", "ws", "ws_bytes", "stream"]
    base = dict(_FACT, **_FACT_N, logdet=None, ws=256, ws_bytes=16)
    rows = _ROWS_FACT_N + [
        (dict(batch=-1), -5), (dict(batch=0), 0), (dict(n=0), 0),
        (dict(ws=None), -8), (dict(ws=16), -8), (dict(ws=None, ws_bytes=1 << 40), -8),
        (dict(ws=None, A=None), -1), (dict(ws=None, n=0), 0),     # the no-op needs no scratch
        (dict(ws_bytes=0), -9), (dict(ws_bytes=16, batch=-1), -5)]
    return "gp_potrf_ws", order, base, -9, rows


def _trtri_table():
    ren = {"A": "L", "lda": "ldl", "strideA": "strideL"}
    order = [ren.get(k, k) for k in _INV_ORDER] + ["stream"]
    base = {ren.get(k, k): v for k, v in _FACT_INV.items()}
    rows = [({ren.get(k, k): v for k, v in change.items()}, rc)
            for change, rc in _rows_fact_inv()]
    return "gp_trtri", order, base, 0, rows


@pytest.mark.parametrize("table", [_potrf_inv_table, _potrf_inv_ws_table, _potrf_table,
                                   _potrf_ws_table, _trtri_table],
                         ids=lambda t: t.__name__.strip("_"))
def test_factorisation_return_codes(lib, table):
    """gp_potrf_inv / _ws, gp_potrf / _ws and gp_trtri: which argument is reported, and in
    which order, before anything is allocated or enqueued."""
    name, order, base, base_rc, rows = table()
    assert sorted(order) == sorted(base), name
    rows = [({}, base_rc)] + rows
    codes = {"gp_potrf": {-1, -2, -3, -4, -5}, "gp_potrf_ws": {-1, -2, -3, -4, -5, -8, -9},
             "gp_potrf_inv_ws": set(range(-8, 0)) | {-11, -12}}.get(name, set(range(-8, 0)))
    assert {rc for _, rc in rows if rc} == codes, name      # every documented code appears
    fn = getattr(lib, name)
    prev = lib.gp_set_potrf_path(0)     # -11 / -12 are the persistent factorisation's scratch
    try:
        got = []
        for change, rc in rows:
            assert set(change) <= set(base), (name, change)
            args = dict(base, **change)
            # a row that passed validation would allocate or launch on the dummy pointers
            assert rc < 0 or args["n"] == 0 or args["batch"] == 0, (name, change)
            got.append(fn(*[args[k] for k in order]))
    finally:
        lib.gp_set_potrf_path(prev)
    assert got == [rc for _, rc in rows], [
        (change, rc, g) for (change, rc), g in zip(rows, got) if g != rc]


# gp_dgemm_ws_bytes(m, n, k): the largest workspace any plan for the size takes (blas.hip
# gemm_plan): split-K slabs of the general kernel (s m n 8 bytes, s the power of two that
# choose_splits picks) or, at n <= 32 and k >= 65536, the tsk slices (ceil(k / kslice) m n 8,
# kslice = ceil(k / max(1, 512 / ceil(m / 256))) rounded up to 16).
_GEMM_WS_BYTES = [
    ((1, 1, 1), 0), ((70, 33, 129), 0), ((17, 5, 60000), 87040),
    ((512, 25, 65535), 6553600), ((512, 25, 65536), 26214400), ((512, 25, 70001), 24985600),
    ((512, 7, 69992), 6995968), ((700, 7, 65537), 6428800), ((512, 33, 70000), 8650752),
    ((300, 32, 65536), 19660800), ((20001, 25, 300), 0), ((25, 20001, 300), 0),
    ((512, 25, 1347945), 26214400), ((0, 5, 5), 0)]


def test_gemm_workspace_bytes(lib):
    got = [lib.gp_dgemm_ws_bytes(*mnk) for mnk, _ in _GEMM_WS_BYTES]
    assert got == [b for _, b in _GEMM_WS_BYTES], [
        (mnk, b, g) for (mnk, b), g in zip(_GEMM_WS_BYTES, got) if g != b]
    for mnk in ((5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, 5, -1)):
        assert lib.gp_dgemm_ws_bytes(*mnk) == 0, mnk


# Return codes of the fit-side entry points of blas.hip, in the form of the tables above: the
# base is a valid no-op (m = 0, ny = 0), so no row reaches a launch; rows with two faults pin
# the order of the checks.
_GEMM_ORDER = ["transa", "transb", "m", "n", "k", "alpha", "A", "a_f32", "lda", "B", "b_f32",
               "ldb", "beta", "C", "ldc", "ws", "ws_bytes", "stream"]
_GEMM_BASE = dict(transa=0, transb=0, m=0, n=5, k=3, alpha=1.0, A=_P, a_f32=0, lda=1, B=_P,
                  b_f32=0, ldb=3, beta=0.0, C=_P, ldc=1, ws=None, ws_bytes=0, stream=None)
_GEMM_M4 = dict(m=4, lda=4, ldc=4)               # m > 0: such a row must fail validation


def _rows_gemm(c):
    """c maps gp_gemm_ex's argument names to the entry point's codes."""
    return [(dict(transa=2), -1), (dict(transa=-1), -1), (dict(transb=2), -2), (dict(m=-1), -3),
            (dict(n=-1), -4), (dict(k=-1), -5), (dict(A=None), c["A"]),
            (dict(A=None, B=None, k=0), 0),                 # k = 0: neither operand is read
            (dict(lda=0), c["lda"]), (dict(_GEMM_M4, lda=3), c["lda"]),
            (dict(transa=1, lda=2), c["lda"]),              # op(A) = A^T: lda >= k
            (dict(transa=1, lda=3), 0),
            (dict(B=None), c["B"]), (dict(ldb=2), c["ldb"]),
            (dict(transb=1, ldb=4), c["ldb"]),              # op(B) = B^T: ldb >= n
            (dict(transb=1, ldb=5), 0),
            (dict(C=None), c["C"]), (dict(ldc=0), c["ldc"]), (dict(_GEMM_M4, ldc=3), c["ldc"]),
            (dict(_GEMM_M4, n=0), 0), (dict(n=0, k=0), 0),
            (dict(transa=2, C=None), -1), (dict(transb=2, m=-1), -2), (dict(m=-1, n=-1), -3),
            (dict(k=-1, A=None), -5), (dict(A=None, lda=0), c["A"]), (dict(lda=0, B=None), c["lda"]),
            (dict(B=None, ldb=2), c["B"]), (dict(ldb=2, C=None), c["ldb"]),
            (dict(C=None, ldc=0), c["C"])]


def _gemm_ex_table():
    c = dict(A=-7, lda=-9, B=-10, ldb=-12, C=-14, ldc=-15)
    rows = _rows_gemm(c) + [(dict(a_f32=2), -8), (dict(a_f32=-1), -8), (dict(b_f32=2), -11),
                            (dict(A=None, a_f32=2), -7), (dict(a_f32=2, lda=0), -8),
                            (dict(B=None, b_f32=2), -10), (dict(b_f32=2, ldb=2), -11),
                            (dict(a_f32=1, b_f32=1), 0)]
    return "gp_gemm_ex", _GEMM_ORDER, _GEMM_BASE, rows


def _dgemm_table():
    """gp_dgemm's own argument numbers: A, lda = 7, 8; B, ldb = 9, 10; C, ldc = 12, 13."""
    c = dict(A=-7, lda=-8, B=-9, ldb=-10, C=-12, ldc=-13)
    order = [k for k in _GEMM_ORDER if k not in ("a_f32", "b_f32")]
    return "gp_dgemm", order, {k: _GEMM_BASE[k] for k in order}, _rows_gemm(c)


def _sim_stats_table():
    order = ["Y", "n", "ny", "ldy", "sd_floor", "mu", "sd", "stream"]
    base = dict(Y=_P, n=3, ny=0, ldy=0, sd_floor=1e-6, mu=_P, sd=_P, stream=None)
    rows = [(dict(Y=None), -1), (dict(n=0), -2), (dict(n=-1), -2), (dict(ny=-1), -3),
            (dict(ny=5, ldy=4), -4), (dict(ldy=-1), -4), (dict(mu=None), -6), (dict(sd=None), -7),
            (dict(n=1), 0), (dict(ldy=7), 0),
            (dict(Y=None, n=0), -1), (dict(n=0, ny=-1), -2), (dict(ny=-1, ldy=-2), -3),
            (dict(ldy=-1, mu=None), -4), (dict(mu=None, sd=None), -6)]
    return "gp_sim_stats", order, base, rows


def _standardize_table():
    order = ["Y", "n", "ny", "ldy", "mu", "sd", "out", "ldo", "inverse", "stream"]
    base = dict(Y=_P, n=3, ny=0, ldy=0, mu=_P, sd=_P, out=_P, ldo=0, inverse=0, stream=None)
    rows = [(dict(Y=None), -1), (dict(n=-1), -2), (dict(ny=-1), -3), (dict(ny=5, ldy=4, ldo=5), -4),
            (dict(ldy=-1), -4), (dict(mu=None), -5), (dict(sd=None), -6), (dict(out=None), -7),
            (dict(ny=5, ldy=5, ldo=4), -8), (dict(ldo=-1), -8),
            (dict(n=0, ny=5, ldy=5, ldo=5), 0), (dict(inverse=1), 0),
            (dict(Y=None, n=-1), -1), (dict(n=-1, ny=-1), -2), (dict(ny=-1, ldy=-2), -3),
            (dict(ldy=-1, mu=None), -4), (dict(mu=None, sd=None), -5), (dict(sd=None, out=None), -6),
            (dict(out=None, ldo=-1), -7)]
    return "gp_standardize", order, base, rows


@pytest.mark.parametrize("table", [_gemm_ex_table, _dgemm_table, _sim_stats_table,
                                   _standardize_table], ids=lambda t: t.__name__.strip("_"))
def test_fitside_return_codes(lib, table):
    """gp_gemm_ex, gp_dgemm, gp_sim_stats and gp_standardize: which argument is reported, and
    in which order, before anything is enqueued."""
    name, order, base, rows = table()
    assert sorted(order) == sorted(base), name
    fn = getattr(lib, name)
    got = []
    for change, rc in [({}, 0)] + rows:
        assert set(change) <= set(base), (name, change)
        args = dict(base, **change)
        # a row that passed validation with work to do would launch on the dummy pointers
        assert rc < 0 or 0 in (args.get("m", 1), args["n"], args.get("ny", 1)), (name, change)
        got.append(fn(*[args[k] for k in order]))
    assert got == [0] + [rc for _, rc in rows], [
        (change, rc, g) for (change, rc), g in zip([({}, 0)] + rows, got) if g != rc]


def test_required_alignment_return_codes(lib):
    """The operands whose alignment the header requires (include/gpfit.h, layout contract): a
    16-B aligned L^-1 / packed P with an even ldinv and strideInv, a 256-B aligned workspace.
    An 8-B-only base, an odd leading dimension and an odd stride each return the argument's
    number before any launch (gp_predict_ex / _solve / _z and gp_fit_predict: _rows_linv)."""
    p16, p8, ws256, ws16 = 16, 8, ctypes.c_void_p(256), ctypes.c_void_p(16)
    order = ["Linv", "ldinv", "strideInv", "X", "ldx", "Xs", "ldxs", "n", "m", "d", "beta",
             "ldbeta", "s", "s_pred", "w_hat", "ldw", "mean", "var", "ldo", "batch", "ws",
             "ws_bytes", "m_chunk", "stream"]
    base = dict(_LINV, **_CROSS, **_OUT, **_WS, stream=None)
    rows = [(dict(), -21), (dict(Linv=p8), -1), (dict(ldinv=_NPAD + 1), -2),
            (dict(strideInv=_NPAD * _NPAD + 1), -3), (dict(strideInv=1, batch=1), -3),
            (dict(ldinv=_NPAD + 2, strideInv=(_NPAD + 2) * _NPAD), -21),   # even: accepted
            (dict(ws=16), -21)]
    for change, want in rows:
        assert lib.gp_predict(*[dict(base, **change)[k] for k in order]) == want, change
    # gp_pack_linv / gp_unpack_linv: both buffers 16-B aligned, ldinv even
    assert lib.gp_pack_linv(p8, 100, 128, p16, None) == -1
    assert lib.gp_pack_linv(p16, 100, 129, p16, None) == -3
    assert lib.gp_pack_linv(p16, 100, 128, p8, None) == -4
    assert lib.gp_unpack_linv(p8, 100, p16, 128, None) == -1
    assert lib.gp_unpack_linv(p16, 100, p8, 128, None) == -3
    assert lib.gp_unpack_linv(p16, 100, p16, 129, None) == -4
    # workspaces: 256-B aligned
    assert lib.gp_potrf_inv_ws(p16, 100, 100, 10000, p16, 128, 128 * 128, 1, None, None, ws16,
                               1 << 30, None) == -11
    assert lib.gp_potrf_ws(p16, 100, 100, 10000, 1, None, None, ws16, 1 << 30, None) == -8
    assert lib.gp_predict_z(p16, 128, 128 * 128, 0, 100, p16, 100, p16, 128, 1, ws16, 1 << 30,
                            None) == -11
    chol = [p16, 100, 10000, p16, 2, p16, 2, 100, 10, 2, p16, 2, p16, p16, p16, 100, p16, p16,
            10, 1, None, ws16, 1 << 40, 0, None]
    assert lib.gp_predict_chol(*chol) == -22
    chol[21] = ws256
    chol[22] = 16
    assert lib.gp_predict_chol(*chol) == -23
    # the factor of gp_predict_chol / gp_trtri and the L^-1 of gp_trmv / gp_nll carry no
    # alignment requirement: an 8-B-only base and odd ld pass validation (no-op sizes here)
    assert lib.gp_trtri(p8, 0, 1, 1, p8, 1, 1, 1, None, None) == 0
    assert lib.gp_trmv(p8, 129, 129 * 128 + 1, 0, p8, 1, p8, 1, 3, None) == 0


def test_mcmc_group_step_validates(lib):
    """gp_mcmc_group_step: both groups' arguments are checked before the launch (the second
    group's prep codes shifted by -10)."""
    from gladsgp_amd import _capi
    S = _capi.McmcState()
    for nm, _ in S._fields_[:14]:
        setattr(S, nm, 64)                           # non-null, never dereferenced here
    S.P, S.d = 4, 2
    T = _capi.McmcState()
    ctypes.pointer(T)[0] = S
    k = (ctypes.c_int * 2)(1, 2)
    dummy = ctypes.c_void_p(64)
    pS, pT = ctypes.addressof(S), ctypes.addressof(T)
    assert lib.gp_mcmc_group_step(None, k, 2, 0, dummy, pT, k, 2, 0, dummy, dummy, dummy,
                                  None) == -1
    assert lib.gp_mcmc_group_step(pS, k, 2, 0, None, pT, k, 2, 0, dummy, dummy, dummy,
                                  None) == -7
    assert lib.gp_mcmc_group_step(pS, k, 2, 0, dummy, None, k, 2, 0, dummy, dummy, dummy,
                                  None) == -11
    bad = (ctypes.c_int * 2)(1, 9)                   # update code > d + 3
    assert lib.gp_mcmc_group_step(pS, k, 2, 0, dummy, pT, bad, 2, 0, dummy, dummy, dummy,
                                  None) == -16
    assert lib.gp_mcmc_group_step(pS, k, 2, 0, dummy, pT, k, 2, 0, None, dummy, dummy,
                                  None) == -17
    T.P = 5
    assert lib.gp_mcmc_group_step(pS, k, 2, 0, dummy, pT, k, 2, 0, dummy, dummy, dummy,
                                  None) == -18


def test_mcmc_group_prep_and_decide_validate(lib):
    """gp_mcmc_group_prep / gp_mcmc_group_decide: every argument code, checked before the
    launch (no pointer here is ever dereferenced)."""
    from gladsgp_amd import _capi
    S = _capi.McmcState()
    for nm, _ in S._fields_[:14]:
        setattr(S, nm, 64)
    S.P, S.d = 4, 2
    pS = ctypes.addressof(S)
    k = (ctypes.c_int * 2)(1, 5)
    dummy = ctypes.c_void_p(64)

    def prep(S_=pS, kinds=k, g=2, beta=dummy, s=dummy, delta=dummy):
        return lib.gp_mcmc_group_prep(S_, kinds, g, 0, beta, s, delta, None)

    def decide(S_=pS, kinds=k, g=2, ll_all=dummy):
        return lib.gp_mcmc_group_decide(S_, kinds, g, 1, ll_all, None)

    for call in (prep, decide):
        assert call(S_=None) == -1
        for P, want in ((0, -2), (1025, -2), (1024, -7), (1, -7)):
            S.P = P                                   # a valid P gets as far as the -7 below
            assert (prep(beta=None) if call is prep else decide(ll_all=None)) == want, P
        S.P = 4
        for d, want in ((0, -3), (33, -3), (32, -7), (1, -6)):     # d = 1: code 5 > d + 3
            S.d = d
            assert (prep(beta=None) if call is prep else decide(ll_all=None)) == want, d
        S.d = 2
        k5 = (ctypes.c_int * 5)(1, 2, 3, 4, 5)
        assert call(g=0) == -4
        assert call(kinds=k5, g=5) == -4
        assert call(kinds=None) == -4
        for nm, _ in S._fields_[:14]:                 # each state pointer in turn
            setattr(S, nm, None)
            assert call() == -5, nm
            setattr(S, nm, 64)
        assert call(kinds=(ctypes.c_int * 2)(1, 0)) == -6
        assert call(kinds=(ctypes.c_int * 2)(0, 1)) == -6
        assert call(kinds=(ctypes.c_int * 2)(1, S.d + 4)) == -6
        assert call(kinds=(ctypes.c_int * 1)(S.d + 4), g=1) == -6
    assert prep(beta=None) == -7
    assert prep(s=None) == -7
    assert prep(delta=None) == -7
    assert decide(ll_all=None) == -7


def test_comm_argument_validation(lib):
    # RCCL wrappers: bad arguments are rejected before librccl is touched
    dummy = ctypes.c_void_p(16)
    assert lib.gp_comm_init(0, 0, dummy, dummy) == -1
    assert lib.gp_comm_init(2, 2, dummy, dummy) == -2
    assert lib.gp_comm_init(1, 0, None, dummy) == -3
    assert lib.gp_comm_unique_id(None) == -1
    assert lib.gp_bcast(None, dummy, 8, 0, None) == -1
    assert lib.gp_gather(None, dummy, 8, dummy, 0, None) == -1
    assert lib.gp_comm_destroy(None) == -1
    assert lib.gp_comm_available() in (0, 1)


def test_product_path_fails_loudly_without_library(monkeypatch, tmp_path):
    from gladsgp_amd import _capi
    monkeypatch.setattr(_capi, "_LIB", None)
    monkeypatch.setattr(_capi, "LIB_PATH", str(tmp_path / "missing.so"))
    with pytest.raises(_capi.GPFitUnavailable):
        _capi.lib()


def test_factorisation_workspace_entry_points(lib):
    """gp_potrf_inv_ws / gp_potrf_ws: sized scratch, validated before any launch; the
    allocating forms validate before allocating."""
    dummy = ctypes.c_void_p(16)
    wsp = ctypes.c_void_p(256)
    inv = lib.gp_potrf_inv_ws_bytes(4096, 1)
    assert inv > 0 and lib.gp_potrf_inv_ws_bytes(4096, 8) > inv
    assert lib.gp_potrf_inv_ws_bytes(-1, 1) == -1
    assert lib.gp_potrf_inv_ws_bytes(64 * 241, 1) == 0          # beyond the persistent kernel
    assert lib.gp_potrf_ws_bytes(512, 4) > lib.gp_potrf_inv_ws_bytes(512, 4)
    # gp_fit_predict / gp_loglik carry the factorisation's scratch in their own workspace
    assert (lib.gp_fit_predict_ws_bytes(4096, 100000, 1, 0) >=
            lib.gp_predict_prepared_ws_bytes(4096, 100000, 1, 0) + inv)
    assert lib.gp_loglik_ws_bytes(512, 8) > lib.gp_potrf_inv_ws_bytes(512, 8)
    assert lib.gp_potrf_inv_ws(None, 10, 10, 100, dummy, 128, 128 * 128, 1, None, None, wsp,
                               1 << 30, None) == -1
    assert lib.gp_potrf_inv_ws(dummy, 100, 100, 10000, dummy, 64, 4096, 1, None, None, wsp,
                               1 << 30, None) == -6
    assert lib.gp_potrf_ws(dummy, 4, 3, 16, 1, None, None, wsp, 1 << 30, None) == -3
    assert lib.gp_potrf_ws(dummy, 0, 1, 0, 1, None, None, None, 0, None) == 0
    assert lib.gp_potrf(dummy, 4, 4, 8, 2, None, None, None) == -4   # before any allocation
    assert lib.gp_loglik_status(None, 4, 1, 0, None) == -1
    assert lib.gp_loglik_status(wsp, 0, 1, 0, None) == 0


def test_schedule_hooks_return_codes(lib):
    """gp_pp_schedule_host / gp_pp_plan / gp_pp_plan_stream / gp_pp_schedule_ws_bytes /
    gp_pp_schedule: minus the argument's position, in argument order, before any launch (no row
    here passes validation of an entry point that would launch or query the device)."""
    from gladsgp_amd import _capi
    wsp, ws16 = ctypes.c_void_p(256), ctypes.c_void_p(16)
    top = 64 * 240
    out3 = (ctypes.c_int * 3)()
    host = lib.gp_pp_schedule_host
    for args, rc in [((0, 1, 0, out3, 1), -1), ((top + 1, 1, 0, out3, 1), -1),
                     ((0, 2, 9, None, -1), -1), ((64, 2, 0, out3, 1), -2),
                     ((64, -1, 9, None, -1), -2), ((64, 1, -1, out3, 1), -3),
                     ((64, 1, 9, None, -1), -3), ((64, 1, 8, None, 1), -4),
                     ((64, 1, 8, None, -1), -5), ((64, 1, 8, out3, -1), -5),
                     ((64, 1, 8, None, 0), 2), ((64, 0, 0, None, 0), 0),
                     ((64, 1, 8, out3, 1), 2)]:
        assert host(*args) == rc, args
    out = (ctypes.c_longlong * len(_capi.PP_PLAN))()
    plan = lib.gp_pp_plan
    for args, rc in [((0, 1, 1, 256, -1, out), -1), ((0, 0, 2, 0, 9, None), -1),
                     ((64, 0, 1, 256, -1, out), -2), ((64, 0, 2, 0, 9, None), -2),
                     ((64, 1, 2, 256, -1, out), -3), ((64, 1, -1, 0, 9, None), -3),
                     ((64, 1, 1, 0, -1, out), -4), ((64, 1, 1, 0, 9, None), -4),
                     ((64, 1, 1, 256, -2, out), -5), ((64, 1, 1, 256, 9, None), -5),
                     ((64, 1, 1, 256, -1, None), -6), ((64, 1, 1, 256, 8, out), 0),
                     ((top + 1, 1, 1, 256, -1, out), 0), ((1 << 30, 1 << 30, 0, 1, 0, out), 0)]:
        assert plan(*args) == rc, args
    assert len(_capi.PP_PLAN) == 12 and list(out)[:2] == [0, 1 << 24]       # not eligible, N
    for args, rc in [((0, 1, 1, -1, out, None), -1), ((64, 0, 1, -1, out, None), -2),
                     ((64, 1, 2, -1, out, None), -3), ((64, 1, 1, -2, out, None), -4),
                     ((64, 1, 1, 9, None, None), -4), ((64, 1, 1, -1, None, None), -5)]:
        assert lib.gp_pp_plan_stream(*args) == rc, args
    size = lib.gp_pp_schedule_ws_bytes
    for args, rc in [((0, 1, 1), -1), ((top + 1, 0, 2), -1), ((64, 0, 1), -2), ((64, 0, 2), -2),
                     ((top, 1 << 20, 1), -2), ((64, 1, 2), -3), ((64, 1, -1), -3)]:
        assert size(*args) == rc, args
    assert size(64, 1, 0) == 256 + 512 and size(top, 8, 1) == lib.gp_potrf_inv_ws_bytes(top, 8)
    sched = lib.gp_pp_schedule
    big = 1 << 40
    for args, rc in [((0, 1, 1, 0, wsp, big, None), -1), ((top + 1, 0, 2, 9, None, 0, None), -1),
                     ((64, 0, 1, 0, wsp, big, None), -2), ((top, 1 << 20, 2, 9, None, 0, None), -2),
                     ((64, 1, 2, 0, wsp, big, None), -3), ((64, 1, -1, 9, None, 0, None), -3),
                     ((64, 1, 1, -1, wsp, big, None), -4), ((64, 1, 1, 9, None, 0, None), -4),
                     ((64, 1, 1, 0, None, big, None), -5), ((64, 1, 1, 0, ws16, big, None), -5),
                     ((64, 1, 1, 0, None, 0, None), -5),
                     ((64, 1, 1, 0, wsp, size(64, 1, 1) - 1, None), -6),
                     ((top, 8, 1, 8, wsp, size(top, 8, 1) - 1, None), -6)]:
        assert sched(*args) == rc, args


def _kernel_resources():
    """Per-kernel register and LDS use read from the built library's gfx950 code objects
    (offload bundles -> AMDGPU metadata note, printed by llvm-readelf)."""
    import re
    import shutil
    import struct
    import subprocess
    import tempfile
    from gladsgp_amd import _build
    readelf = shutil.which("llvm-readelf") or "/opt/rocm/llvm/bin/llvm-readelf"
    if not os.path.exists(_build.LIB_PATH) or not os.path.exists(readelf):
        pytest.skip("built library or llvm-readelf missing")
    data = open(_build.LIB_PATH, "rb").read()
    out, pos = {}, 0
    while True:
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", pos)
        if i < 0:
            break
        pos = i + 24
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl].decode(errors="replace")
            p += tl
            if "gfx950" not in triple or not size:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(data[i + off:i + off + size])
                f.flush()
                notes = subprocess.run([readelf, "--notes", f.name], capture_output=True,
                                       text=True, check=True).stdout
            for blk in notes.split("\n  - ")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if not name:
                    continue
                g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))  # noqa
                out[name.group(1)] = {"vgpr": g("vgpr_count"), "agpr": g("agpr_count"),
                                      "lds": g("group_segment_fixed_size")}
    return out


def _alloc(r):
    """Registers a wave of the kernel holds per lane on gfx950 (unified VGPR/AGPR file: the
    metadata's .vgpr_count is the total, arch VGPRs + AGPRs), in granules of 8."""
    return -(-r["vgpr"] // 8) * 8


def test_persistent_factorisation_leaves_room_for_cross():
    """gp_fit_predict runs the cross-covariance (cross_kp_kernel<8>, every d <= 8 config) beside
    the persistent factorisation (pp_kernel, one 4-wave workgroup per CU); that overlap exists
    only while one wave of each fits on a SIMD: registers <= 512 per lane, LDS <= 160 KB per CU.
    Round 4 found it broken by 10 extra pp_kernel registers (C3 27.7 vs 26.8 ms per step: the
    cross-covariance waited for the whole factorisation) -- this guards the budget."""
    res = _kernel_resources()
    # pp_kernel<false>: the factorisation gp_fit_predict overlaps (pp_kernel<true> is
    # gp_loglik's in-chain mode, which runs with no cross-covariance beside it)
    pp = [v for k, v in res.items() if "pp_kernelILb0E" in k]
    cross = [v for k, v in res.items() if "cross_kp_kernelILi8E" in k]
    assert pp and cross, sorted(res)[:20]
    pp, cross = pp[0], cross[0]
    assert _alloc(pp) + _alloc(cross) <= 512, (pp, cross, _alloc(pp), _alloc(cross))
    assert pp["lds"] + cross["lds"] <= 160 * 1024, (pp, cross)


@pytest.mark.parametrize("seed,pre,shape", [
    (0, 0, (1,)), (0, 1, (1,)), (1, 0, (2,)), (2, 3, (3,)), (3, 0, (7, 5)), (4, 5, (1000,)),
    (5, 0, (624,)), (6, 623, (20001,)), (7, 0, (3000, 50)), (8, 311, (157,)), (9, 2, (0,)),
    # above 2 x kBatch (2^20 accepted pairs = 2^21 deviates per batch, host_rng.hip): the
    # double-buffered path -- flush(false), buffer swap, one batch's transform threads beside
    # the next batch's fill -- runs several times, as it does for the fit's 1.35M x 25 Omega
    (10, 7, (4_300_001,))])
def test_legacy_normal_matches_numpy(seed, pre, shape):
    """svd.legacy_normal_f32 (gp_host_legacy_normal_f32, host code: no GPU) == the reference's
    np.random.normal(size=...).astype(np.float32) (src/svd.py:51) bit for bit, from any
    generator position (pre draws: odd counts leave a cached deviate, pos anywhere in a twist),
    and numpy's global state afterwards equals the state numpy's own call leaves."""
    from gladsgp_amd.svd import legacy_normal_f32
    np.random.seed(seed)
    np.random.normal(size=pre)
    st = np.random.get_state()
    ref = np.random.normal(size=shape).astype(np.float32)
    st_ref = np.random.get_state()
    np.random.set_state(st)
    got = legacy_normal_f32(shape, threads=3)
    st_got = np.random.get_state()
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(st_got[1], st_ref[1]) and st_got[2:] == st_ref[2:]


def test_legacy_normal_draw_on_worker_thread():
    """svd.LegacyNormalDraw (init_model's Omega, drawn beside the upload): the same deviates as
    the reference's np.random.normal((ny, 25)).astype(float32) (src/svd.py:51), numpy's global
    state read on the calling thread when the draw starts and advanced there by result()."""
    from gladsgp_amd.svd import LegacyNormalDraw
    np.random.seed(11)
    st0 = np.random.get_state()
    ref = np.random.normal(size=(30001, 25)).astype(np.float32)
    st_ref = np.random.get_state()
    np.random.set_state(st0)
    draw = LegacyNormalDraw((30001, 25), threads=2)
    got = draw.result()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    st = np.random.get_state()
    assert np.array_equal(st[1], st_ref[1]) and st[2:] == st_ref[2:]
    assert draw.result() is got                 # result() advances the state once
    assert np.array_equal(np.random.get_state()[1], st_ref[1])


def test_legacy_normal_argument_validation(lib):
    key = (ctypes.c_uint * 624)()
    pos, hg, g = ctypes.c_int(624), ctypes.c_int(0), ctypes.c_double(0.0)
    out = (ctypes.c_float * 4)()
    f = lib.gp_host_legacy_normal_f32
    assert f(None, ctypes.byref(pos), ctypes.byref(hg), ctypes.byref(g), 4, out, 1) == -1
    bad = ctypes.c_int(625)
    assert f(key, ctypes.byref(bad), ctypes.byref(hg), ctypes.byref(g), 4, out, 1) == -2
    assert f(key, ctypes.byref(pos), ctypes.byref(hg), ctypes.byref(g), -1, out, 1) == -5
    assert f(key, ctypes.byref(pos), ctypes.byref(hg), ctypes.byref(g), 4, None, 1) == -6


def test_legacy_normal_reproduces_the_reference_omega():
    """The golden test matrices drawn by the reference's own src/svd.py:51 after
    np.random.seed(123) (tests/golden/svd_ref_64x500.npz, make_golden.py) come out of
    svd.legacy_normal_f32 bit for bit after the same seed."""
    from gladsgp_amd.svd import legacy_normal_f32
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "svd_ref_64x500.npz"))
    for tag in ("p8", "p25k0"):
        ref = g[f"{tag}_omega"]
        np.random.seed(123)
        got = legacy_normal_f32(ref.shape, threads=4)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), tag


def test_predict_workspace_holds_the_merged_tail(lib):
    """gp_predict sizes two cross-covariance slabs exactly when the last chunk is partial (so it
    can run merged with the chunk before it), one otherwise."""
    full = lib.gp_predict_ws_bytes(1000, 32768, 1, 0)
    part = lib.gp_predict_ws_bytes(1000, 32768 + 128, 1, 0)
    one = lib.gp_predict_ws_bytes(1000, 16384, 1, 0)
    slab = 8 * 1024 * 16384                         # npad x chunk doubles
    assert part - full >= slab                      # the second slab (+ partial sums)
    assert full == one                              # whole chunks reuse one slab

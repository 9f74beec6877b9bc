"""CPU: every documented return code of gp_mcmc_ens_prep / _decide / _step (include/gpfit.h),
checked before any launch: no pointer here is ever dereferenced and no device work happens."""
import ctypes

import pytest

NPTR = 14                                  # pointer fields of gp_mcmc_state / gp_mcmc_strides
SHARED = ("lam", "u", "step_betaU", "step_lamUz", "step_lamWs", "step_lamWOs")
P, D = 4, 2


@pytest.fixture(scope="module")
def lib():
    from gladsgp_amd import _build, _capi
    _build.build_library()
    return _capi.lib()


def _state(P_=P, d=D):
    from gladsgp_amd import _capi
    S = _capi.McmcState()
    for nm, _ in S._fields_[:NPTR]:
        setattr(S, nm, 64)                 # non-null, never dereferenced
    S.P, S.d = P_, d
    return S


def _extents(P_=P, d=D):
    from gladsgp_amd import _capi
    return dict(betaU=(d + 1) * P_, lamUz=P_, lamWs=P_, lamWOs=1, ll=P_, acc=(d + 4) * P_, lp=1,
                scratch=3 * _capi.MCMC_MAX_GROUP * P_)


def _strides(**change):
    """Packed strides (every written buffer exactly its extent, the shared ones 0)."""
    from gladsgp_amd import _capi
    T = _capi.McmcStrides()
    for nm, v in _extents().items():
        setattr(T, nm, v)
    for nm, v in change.items():
        setattr(T, nm, v)
    return T


def _calls(lib):
    """prep / decide / step as functions of the arguments the codes -1 .. -9 name; valid
    defaults reach a launch, so every call here breaks at least one of them."""
    S, T = _state(), _strides()
    k = (ctypes.c_int * 2)(1, D + 3)
    dummy = ctypes.c_void_p(64)

    def prep(S_=S, T_=T, C=2, kinds=k, g=2, out=dummy):
        return lib.gp_mcmc_ens_prep(ctypes.addressof(S_) if S_ is not None else None,
                                    ctypes.addressof(T_) if T_ is not None else None, C, kinds,
                                    g, 0, out, dummy, dummy, None)

    def decide(S_=S, T_=T, C=2, kinds=k, g=2, out=dummy):
        return lib.gp_mcmc_ens_decide(ctypes.addressof(S_) if S_ is not None else None,
                                      ctypes.addressof(T_) if T_ is not None else None, C,
                                      kinds, g, 1, out, None)

    def step(S_=S, T_=T, C=2, kinds=k, g=2, out=dummy):
        # `out` is the decided group's ll_all; the next group is valid up to its null beta
        return lib.gp_mcmc_ens_step(ctypes.addressof(S_) if S_ is not None else None,
                                    ctypes.addressof(T_) if T_ is not None else None, C, kinds,
                                    g, 0, out, ctypes.addressof(S), k, 2, 0, None, dummy, dummy,
                                    None)

    return S, prep, decide, step


@pytest.mark.parametrize("which", ["prep", "decide", "step"])
def test_first_group_codes(lib, which):
    """-1 .. -9 in the documented order; a call with nothing wrong but a null output gets as far
    as -7 (prep, decide) or the next group's -17 (step)."""
    from gladsgp_amd import _capi
    S, prep, decide, step = _calls(lib)
    call = dict(prep=prep, decide=decide, step=step)[which]
    assert call(S_=None) == -1
    for bad in (0, 1025):
        assert call(S_=_state(P_=bad)) == -2
    for bad in (0, 33):
        assert call(S_=_state(d=bad)) == -3
    assert call(g=0) == -4
    assert call(kinds=(ctypes.c_int * 5)(1, 2, 3, 4, 5), g=5) == -4
    assert call(kinds=None) == -4
    for nm, _ in S._fields_[:NPTR]:
        bad = _state()
        setattr(bad, nm, None)
        assert call(S_=bad) == -5, nm
    for kinds in ((1, 0), (0, 1), (1, D + 4)):
        assert call(kinds=(ctypes.c_int * 2)(*kinds)) == -6
    assert call(out=None) == -7
    for C in (0, -1, _capi.MCMC_MAX_CHAINS + 1):
        assert call(C=C) == -8, C
    assert call(T_=None) == -9
    assert call(T_=None, C=1) == -9                    # one chain still needs the struct
    for nm, ext in _extents().items():                 # a written buffer: no sharing, no overlap
        assert call(T_=_strides(**{nm: 0})) == -9, nm
        assert call(T_=_strides(**{nm: ext - 1})) == -9, nm
        assert call(T_=_strides(**{nm: -ext})) == -9, nm
    for nm in SHARED:
        assert call(T_=_strides(**{nm: -1})) == -9, nm
    # the order of the checks: the earlier argument is the one reported
    assert call(S_=None, C=0) == -1
    assert call(out=None, C=0) == -7
    assert call(C=0, T_=None) == -8
    assert call(kinds=(ctypes.c_int * 2)(1, 0), out=None) == -6
    # nothing wrong: one chain never reads the strides; the largest ensemble; shared, padded and
    # overlapping read-only strides.  gp_mcmc_ens_step reports its next group's null beta (-17)
    # only after it has accepted all of these (prep and decide would launch: the GPU tests
    # run them with such strides)
    if which == "step":
        for kw in (dict(C=1, T_=_strides(betaU=0, ll=-5)), dict(C=_capi.MCMC_MAX_CHAINS),
                   dict(T_=_strides(lam=P, u=7, betaU=1000, lp=1))):
            assert call(**kw) == -17, kw


def test_step_second_group_codes(lib):
    """gp_mcmc_ens_step: the next group's prep codes shifted by -10, then -18 and -19."""
    S, T = _state(), _strides()
    k = (ctypes.c_int * 2)(1, 2)
    dummy = ctypes.c_void_p(64)

    def step(Sn=S, kn=k, gn=2, beta=dummy, s=dummy, delta=dummy, S_=S, T_=T, C=2):
        return lib.gp_mcmc_ens_step(ctypes.addressof(S_), ctypes.addressof(T_), C, k, 2, 0,
                                    dummy, ctypes.addressof(Sn) if Sn is not None else None,
                                    kn, gn, 0, beta, s, delta, None)

    assert step(Sn=None) == -11
    assert step(Sn=_state(P_=0)) == -12
    assert step(Sn=_state(d=33)) == -13
    assert step(gn=0) == -14
    assert step(kn=None) == -14
    bad = _state()
    bad.lam = None
    assert step(Sn=bad) == -15
    assert step(kn=(ctypes.c_int * 2)(1, 9)) == -16
    for kw in (dict(beta=None), dict(s=None), dict(delta=None)):
        assert step(**kw) == -17
    assert step(Sn=_state(P_=5)) == -18
    # the one strides struct must also suit S_next: d = 5 needs betaU >= 6 P and acc >= 9 P
    assert step(Sn=_state(d=5)) == -19
    assert step(Sn=_state(d=5), C=1, beta=None) == -17     # one chain: strides not read
    # the decided group's codes come first
    assert step(Sn=None, C=0) == -8
    assert step(Sn=None, T_=_strides(ll=0)) == -9

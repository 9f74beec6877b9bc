"""CPU: the persistent factorisation's task list and launch rule against a dependence model.

pp_kernel's workgroups dequeue one task list strictly in order and spin on per-tile flags, so
the list's order and the rule that sizes the launch (pp_plan in gladsgp_amd/csrc/chol.hip) are
what keeps a launch from hanging.  The library's host hooks give the list (gp_pp_schedule_host,
the same pp_for_key the schedule kernel runs) and the rule (gp_pp_plan, the function the entry
points launch from); tests/_pp_sched_ref.py is the model.  No device work happens here;
tests/test_gpu_pp_sched.py checks that the device emits exactly this list.

"stuck" is the largest number of one problem's dequeued tasks that cannot complete from the
prefix dequeued so far (plus its chain).  Measured with this model for every N in 1..48 and
63, 64, 65, 127, 128, 129, 239, 240, with and without L^-1:
  lead W = 0:            stuck = 0  (the list is topological)
  lead W = kPPLead = 4:  stuck = 13 (0 for N <= 4; 4 / 8 / 12 at N = 5 / 6 / 7; 13 from N = 8 on)
against the rule's bound kPPLeadBlocked = 22.  At N = 16 and N = 40, W = 1, 2, 4, 6, 8 give
1, 5, 13, 21, 29.
"""
import ctypes

import numpy as np
import pytest

import _pp_sched_ref as ref

SIZES = list(range(1, 49)) + [63, 64, 65, 127, 128, 129, 239, 240]


@pytest.fixture(scope="module")
def lib():
    from gladsgp_amd import _build, _capi
    _build.build_library()
    return _capi.lib()


def host_list(lib, N, inv, lead, n=None):
    """One problem's (kind, i, j) triples in emission order."""
    n = 64 * N if n is None else n
    count = lib.gp_pp_schedule_host(n, inv, lead, None, 0)
    assert count >= 0, count
    buf = np.full((count + 1, 3), -7, dtype=np.int32)
    assert lib.gp_pp_schedule_host(n, inv, lead, buf.ctypes.data, count) == count
    assert np.all(buf[count] == -7)                  # nothing past `cap`
    return buf[:count].astype(np.int64)


def plan(lib, n, batch, inv, resident, lead=-1):
    from gladsgp_amd import _capi
    out = (ctypes.c_longlong * len(_capi.PP_PLAN))()
    assert lib.gp_pp_plan(n, batch, inv, resident, lead, out) == 0
    return dict(zip(_capi.PP_PLAN, out))


def _align256(x):
    return (x + 255) // 256 * 256


def _scratch_bytes(N, batch, tasks):
    """The documented scratch layout (include/gpfit.h, gp_pp_schedule)."""
    fstride = (2 * N * N + 2 * N + 1 + 31) // 32 * 32
    return _align256((tasks + 1) * batch * 8) + _align256(256 + batch * fstride * 4)


@pytest.fixture(scope="module")
def consts(lib):
    p = plan(lib, 64, 1, 1, 256)
    assert p["kPPLead"] > 0 and p["kPPLeadBlocked"] > 0 and p["kPPMaxN"] == 240
    return p


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("N", SIZES)
def test_list_is_complete_and_its_stuck_count_is_bounded(lib, consts, N, inv):
    W, bound = consts["kPPLead"], consts["kPPLeadBlocked"]
    for n in (64 * N, 64 * (N - 1) + 1):             # a full last tile, a last tile of one row
        counts = {lead: lib.gp_pp_schedule_host(n, inv, lead, None, 0) for lead in range(9)}
        assert len(set(counts.values())) == 1, counts            # the same for every lead
        p = plan(lib, n, 1, inv, 256)
        assert p["N"] == N and p["tasks"] == counts[0] and p["nkeys"] <= 1024
    for batch in (1, 3, 8):
        pers = _scratch_bytes(N, batch, counts[0])
        assert lib.gp_pp_schedule_ws_bytes(64 * N, batch, inv) == pers
        if inv:
            assert lib.gp_potrf_inv_ws_bytes(64 * N, batch) == pers
        else:
            assert lib.gp_potrf_ws_bytes(64 * N, batch) == _align256(8 * 64 * 64 * N * batch) + pers
    for lead in (0, W):
        t = host_list(lib, N, inv, lead)
        assert len(t) == counts[0]
        assert ref.complete_errors(t, N, inv) == []
        prof = ref.profile(ref.single(t), N, chains_running=True)
        print(f"N={N} inv={inv} lead={lead}: tasks {len(t)}, max stuck {prof.max_stuck}")
        assert prof.final_blocked == 0
        assert prof.max_stuck == 0 if lead == 0 else prof.max_stuck <= bound, prof.max_stuck


def test_shape_limit_and_key_count(lib, consts):
    top = 64 * consts["kPPMaxN"]
    for inv in (0, 1):
        p = plan(lib, top, 1, inv, 256)
        assert p["eligible"] == 1 and p["N"] == consts["kPPMaxN"]
        assert p["lead"] == consts["kPPLead"] and p["nkeys"] <= 1024
        assert plan(lib, top, 1, inv, 256, lead=8)["nkeys"] <= 1024
        q = plan(lib, top + 1, 1, inv, 256)
        assert q["eligible"] == 0 and (q["grid"], q["groups"], q["tasks"]) == (0, 0, 0)
        assert lib.gp_pp_schedule_host(top + 1, inv, 0, None, 0) == -1
        assert lib.gp_pp_schedule_ws_bytes(top + 1, 1, inv) == -1
    # a batch too small for its chains and as many workers again takes the blocked sweep
    assert plan(lib, 512, 129, 1, 256)["eligible"] == 0
    assert plan(lib, 512, 128, 1, 256)["eligible"] == 1
    prev = lib.gp_set_potrf_path(1)
    try:
        assert plan(lib, 512, 8, 1, 256)["eligible"] == 0
        lib.gp_set_potrf_path(2)
        assert plan(lib, 512, 8, 1, 256)["groups"] == 1
    finally:
        lib.gp_set_potrf_path(prev)
    assert plan(lib, 512, 8, 1, 256)["groups"] == 8


def test_model_rejects_larger_leads(lib, consts):
    """The stuck count grows with the lead and passes the rule's bound: the bound belongs to
    kPPLead, and the model is what would say so if the lead were raised."""
    for N in (16, 40):
        s = [ref.profile(ref.single(host_list(lib, N, 1, W)), N, chains_running=True).max_stuck
             for W in range(9)]
        print(f"N={N}: max stuck by lead {s}")
        assert s[0] == 0 and all(a < b for a, b in zip(s, s[1:]))
        assert s[consts["kPPLead"]] <= consts["kPPLeadBlocked"] < s[8]


RESIDENT = list(range(8, 321, 8)) + [1, 3, 7, 23, 47, 255, 257, 303]


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("N", [2, 5, 9])
def test_launch_rule_never_deadlocks_the_batched_list(lib, consts, N, inv):
    """Every (batch, residency) the rule lets onto the persistent kernel, with the lead, grid
    and queues it picks, against the model on the real interleaved list and its queues."""
    W, bound = consts["kPPLead"], consts["kPPLeadBlocked"]
    lists = {lead: host_list(lib, N, inv, lead) for lead in (0, W)}
    cache = {}

    def queues(batch, lead, groups):
        key = (batch, lead, groups)
        if key not in cache:
            e = ref.batched(lists[lead], batch)
            assert ref.layout_errors(e, batch, groups) == []
            assert np.array_equal(ref.decode(ref.encode(e)), e)
            profs = ref.queue_profiles(e, N, groups)
            assert all(p.final_blocked == 0 for p in profs)
            cache[key] = (max(p.max_blocked for p in profs), max(p.max_stuck for p in profs))
        return cache[key]

    seen = {"eligible": 0, "lead": 0, "groups": 0}
    for batch in range(1, 301):
        for resident in RESIDENT:
            p = plan(lib, 64 * N, batch, inv, resident)
            total = batch * (p["tasks"] + 1)
            assert p["groups"] in (1, 8) and p["lead"] in (0, W)
            assert 1 <= p["grid"] <= min(resident, total)
            if p["groups"] == 8:
                assert batch % 8 == 0 and p["grid"] % 8 == 0
            if p["lead"] > 0:
                assert batch * (bound + 1) < p["grid"]
            if not p["eligible"]:
                continue
            seen["eligible"] += 1
            seen["lead"] += p["lead"] > 0
            seen["groups"] += p["groups"] == 8
            blocked, stuck = queues(batch, p["lead"], p["groups"])
            G, B = p["grid"] // p["groups"], batch // p["groups"]
            assert blocked < G, (batch, resident, p, blocked)
            if p["grid"] < total:          # fewer workgroups than entries: chains hold B of them
                assert stuck < G - B, (batch, resident, p, stuck)
    # (a problem of fewer than `bound` tasks never has the entries for a grid that allows a lead)
    assert seen["eligible"] > 0 and seen["groups"] > 0, seen
    assert (seen["lead"] > 0) == (len(lists[0]) > bound), seen


@pytest.mark.parametrize("inv", [0, 1])
def test_launch_rule_against_the_per_problem_bound(lib, consts, inv):
    """N = 40: every problem's stuck tasks and its chain fit in the grid (or in its queue's share
    of both) with a workgroup to spare."""
    N, W = 40, consts["kPPLead"]
    stuck = {lead: ref.profile(ref.single(host_list(lib, N, inv, lead)), N,
                               chains_running=True).max_stuck for lead in (0, W)}
    eligible = 0
    for batch in range(1, 301):
        for resident in RESIDENT:
            p = plan(lib, 64 * N, batch, inv, resident)
            if p["groups"] == 8:
                assert batch % 8 == 0 and p["grid"] % 8 == 0
            if p["lead"] > 0:
                assert batch * (consts["kPPLeadBlocked"] + 1) < p["grid"]
            if p["eligible"]:
                eligible += 1
                G, B = p["grid"] // p["groups"], batch // p["groups"]
                assert B * (stuck[p["lead"]] + 1) < G, (batch, resident, p)
    assert eligible > 0


# ---- the model must have teeth: lists mutated here, nothing touches a GPU ---------------------

def _find(t, kind, i, j):
    hit = np.flatnonzero((t[:, 0] == kind) & (t[:, 1] == i) & (t[:, 2] == j))
    assert len(hit) == 1, (kind, i, j)
    return int(hit[0])


def _stuck(t, N):
    return ref.profile(ref.single(t), N, chains_running=True)


@pytest.mark.parametrize("N", [9, 16])
def test_model_reports_a_dropped_task(lib, N):
    t = host_list(lib, N, 1, 0)
    kinds = sorted(set(t[:, 0].tolist()))
    assert set(kinds) >= {ref.LT, ref.DP, ref.SP, ref.XT, ref.Z}
    assert (ref.ZP in kinds) == (N % 2 == 1) and (ref.XT2 in kinds) == (N > 10)
    for k in kinds:
        for at in np.flatnonzero(t[:, 0] == k)[[0, -1]]:
            cut = np.delete(t, at, axis=0)
            assert any("missing" in e for e in ref.complete_errors(cut, N, 1)), (k, at)
            if k in (ref.LT, ref.DP, ref.SP) or (k in (ref.XT, ref.XT2) and t[at, 1] < N - 1):
                # somebody waits for it for ever (the last row's L^-1 tiles have no reader)
                assert _stuck(cut, N).final_blocked > 0, (k, at)
            elif k in (ref.Z, ref.ZP):
                assert _stuck(cut, N).final_blocked == 0


@pytest.mark.parametrize("N", [9, 16])
def test_model_reports_a_duplicated_task(lib, N):
    t = host_list(lib, N, 1, 0)
    for k in sorted(set(t[:, 0].tolist())):
        at = np.flatnonzero(t[:, 0] == k)[0]
        dup = np.insert(t, at, t[at], axis=0)
        assert any("times" in e for e in ref.complete_errors(dup, N, 1)), k


def test_model_reports_an_lt_ahead_of_its_producer(lib):
    """Lead 0: every LT(i, j) with j >= 1 swapped with the task that produces its input
    L(i, j-1) leaves the list complete but no longer topological."""
    N = 9
    t = host_list(lib, N, 1, 0)
    assert _stuck(t, N).max_stuck == 0
    moved = 0
    for i in range(3, N):
        for j in range(1, i - 1):
            a, b = _find(t, ref.LT, i, j - 1), _find(t, ref.LT, i, j)
            assert a < b
            mut = t.copy()
            mut[[a, b]] = mut[[b, a]]
            assert ref.complete_errors(mut, N, 1) == []
            prof = _stuck(mut, N)
            assert prof.max_stuck >= 1 and prof.final_blocked == 0, (i, j)
            # a launch of one chain and one worker hangs on it; the real order does not
            assert ref.launch_deadlocks(ref.batched(mut, 1), N, 2, 1)
            moved += 1
    assert moved > 10
    assert not ref.launch_deadlocks(ref.batched(t, 1), N, 2, 1)


@pytest.mark.parametrize("N", [9, 16])
def test_model_reports_reversed_xt_rows(lib, N):
    t = host_list(lib, N, 1, 0)
    xt = np.flatnonzero((t[:, 0] == ref.XT) | (t[:, 0] == ref.XT2))
    rows = t[xt]
    assert np.all(np.diff(rows[:, 1]) >= 0)                      # emitted by ascending row
    mut = t.copy()
    mut[xt] = rows[np.argsort(-rows[:, 1], kind="stable")]
    assert ref.complete_errors(mut, N, 1) == []
    prof = _stuck(mut, N)
    print(f"N={N}: reversed XT rows, max stuck {prof.max_stuck}")
    assert prof.max_stuck >= 1 and prof.final_blocked == 0
    assert ref.launch_deadlocks(ref.batched(mut, 1), N, 2, 1)
    assert not ref.launch_deadlocks(ref.batched(t, 1), N, 2, 1)


def test_model_reports_the_historical_deadlock(lib, consts):
    """n = 1024 (N = 16), batch 32 on 256 workgroups with lead 6 for every problem hung; the
    rule now gives that launch lead 0."""
    N, batch, grid = 16, 32, 256
    one = _stuck(host_list(lib, N, 1, 6), N).max_stuck
    assert one == 21
    e = ref.batched(host_list(lib, N, 1, 6), batch)
    assert ref.profile(e, N).max_stuck == batch * one >= grid - batch
    assert ref.launch_deadlocks(e, N, grid, 1)
    assert ref.launch_deadlocks(e, N, grid, 8)
    p = plan(lib, 1024, batch, 1, grid)
    assert (p["eligible"], p["lead"], p["grid"], p["groups"]) == (1, 0, grid, 8)
    ok = ref.batched(host_list(lib, N, 1, p["lead"]), batch)
    assert not ref.launch_deadlocks(ok, N, grid, 8)
    assert not ref.launch_deadlocks(ok, N, grid, 1)
    # the lead the library would use where it allows one needs batch x (bound + 1) < grid
    lead4 = ref.batched(host_list(lib, N, 1, consts["kPPLead"]), batch)
    assert ref.launch_deadlocks(lead4, N, grid, 8)
    assert plan(lib, 1024, 11, 1, grid)["lead"] == consts["kPPLead"]
    assert plan(lib, 1024, 12, 1, grid)["lead"] == 0

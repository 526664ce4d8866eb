"""GPU tests of the reduced-space minimize call (dto_projected_minimize and its _dev form; csrc/dto_minimize.hip, csrc/dto_minimize_plan.h).

Bits: the one call equals minimize_cases.minimize_loop -- the header's loop restated in NumPy -- composed from the PUBLIC host methods
(preconditioned_newton_step / auglag_newton_step, auglag_merit, auglag_rows): Z, mu, rho, info, both histories and the last step's entry
states, on both "reduced_input_store" routes, in both entry-point families and on a repeated call.
Shapes: 41 entries (one chunk), 12 x 66 (more than one chunk), 40 x 258 (11610 entries: 46 chunks, three workgroups, the last chunk
ragged); 11, 69 (more than one wavefront) and 299 (more than one chunk) penalised rows.  At least three trials everywhere, so both banks
of scalars are read and written.
Values: the one call makes the decisions of the oracle's runs (minimize_cases / auglag_cases); no new bar is set."""
import functools

import numpy as np
import pytest

import auglag_cases as A
import dto_amd
import long_cases as LC
import minimize_cases as M
import newton_box_cases as B
import reduced_cases as R
from helpers import to_engine
from test_gpu_newton_step import REBUILD_NAMES, device_arrays, launches

pytestmark = pytest.mark.gpu

SIGMA = R.SIGMA
# name -> (outer, trials, options); rho = None
PLAIN = {"scaled_12x9+con": (1, 10, dict(rtol=1e-6)), "scaled_12x66+con": (1, 4, dict(max_iter=8)), "scaled_40x258": (1, 4, dict(max_iter=8))}
# with rho
PENALISED = {"al_12x9": (5, 10, dict(A.STEP_KW)), "al_8x70": (2, 3, dict(A.STEP_KW, max_iter=6)), "al_8x300": (2, 3, dict(A.STEP_KW, max_iter=6))}


@functools.lru_cache(maxsize=None)
def case_of(name):
    """the problems, the start, mu, rho and the box"""
    if name in PENALISED:
        c = A.case(name, dense=False)
        n_rows = c["n_cons"] - c["n_dyn"]
        return dict(pe=c["pe"], kw=c["kw"], p=c["p"], Z=c["Z"], mu=np.zeros(c["n_cons"]), rho=A.full(c["n_dyn"], np.full(n_rows, A.RHO)), n_dyn=c["n_dyn"],
                    lo=None, hi=None)
    if name == "scaled_12x9+con":
        c = R.case(name)
        return dict(pe=c["pe"], kw=c["kw"], p=c["p"], Z=c["Z"], mu=c["mu"], rho=None, n_dyn=c["n_dyn"], lo="box", hi="box")
    p, kw = R.problem(name)
    Z = LC.long_point(p)
    Z.setflags(write=False)
    n_dyn = sum(it.x_dim for it in p.integrators) * (p.N - 1)
    n_cons = n_dyn + sum(k.g_dim * len(k.times1) for k in p.constraints)
    mu = None
    if name.endswith("+con"):
        mu = np.zeros(n_cons)
        mu[n_dyn:] = np.random.default_rng(11).standard_normal(n_cons - n_dyn)
    return dict(pe=to_engine(p), kw=kw, p=p, Z=Z, mu=mu, rho=None, n_dyn=n_dyn, lo=None, hi=None)


def evaluator(c, store, pairs=0):
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    if store:
        ev.set_option("reduced_input_store", 1)
    if pairs:
        ev.set_option("newton_pairs", pairs)
    return ev


def start_of(ev, c):
    """(Z0, lo, hi): the box of the use test is built around the engine's feasible start"""
    if c["lo"] is None:
        return np.array(c["Z"]), None, None
    Z0 = ev.feasible_trajectory_engine(c["Z"])
    lo, hi = B.loop_box(Z0, R.index_sets(c["p"])[1], 0.3)
    return Z0, lo, hi


def composed_callables(ev, lo, hi, opt, pairs=0, harvest=False):
    """minimize_loop's callables from the public host methods"""
    kw = M.step_kw(opt)

    def step(Z, delta, mu, rho):
        if pairs:
            _, info, es, zp = ev.preconditioned_newton_step(Z, SIGMA, mu, rho, lo, hi, radius=delta, harvest=harvest, states=True, trajectory=True, **kw)
        else:
            _, info, es, zp = ev.auglag_newton_step(Z, SIGMA, mu, rho, lo, hi, radius=delta, states=True, trajectory=True, **kw)
        return info["raw"], zp, es

    def merit(Z, mu, rho):
        return ev.auglag_merit(Z, SIGMA, mu, rho, trajectory=True)

    def rows(Z, mu, rho):
        mu_eff, _, info = ev.auglag_rows(Z, mu, rho)
        return mu_eff, info["raw"]

    return step, merit, rows


def settings(name, over=None):
    outer, trials, okw = dict(PLAIN, **PENALISED)[name]
    return outer, trials, dict(okw, **(over or {}))


@functools.lru_cache(maxsize=None)
def composed(name, store, pairs=0, harvest=False, over=()):
    """the restatement around the public host methods, once per run"""
    c = case_of(name)
    outer, trials, okw = settings(name, dict(over))
    outer, trials = okw.pop("outer", outer), okw.pop("trials", trials)
    opt = M.options(**okw)
    ev = evaluator(c, store, pairs)
    try:
        Z0, lo, hi = start_of(ev, c)
        step, merit, rows = composed_callables(ev, lo, hi, opt, pairs, harvest)
        run = M.minimize_loop(step, merit, rows, Z0, c["mu"], c["rho"], c["n_dyn"], opt, outer, trials, 16 if pairs else 12)
    finally:
        ev.close()
    return dict(run, lo=lo, hi=hi, Z0=Z0)


def one_call(ev, c, name, family, Z0, lo, hi, pairs=0, harvest=False, over=None):
    """the call through one entry-point family, as the dict minimize_loop returns"""
    outer, trials, okw = settings(name, over)
    outer, trials = okw.pop("outer", outer), okw.pop("trials", trials)
    mu, rho = c["mu"], c["rho"]
    if family == "host":
        out = ev.reduced_minimize(Z0, SIGMA, mu, rho, lo, hi, outer=outer, trials=trials, harvest=harvest, history=True, states=True, **okw)
        Z, info = out[0], out[1]
        mu_o, rho_o = (out[2], out[3]) if rho is not None else (mu, None)
        hist, ohist, es = out[-3], out[-2], out[-1]
        return dict(Z=Z, mu=mu_o, rho=rho_o, info=info["raw"], history=hist, outer_history=ohist, states=es, named=info)
    n, nc = Z0.size, ev.n_constraints
    arrays = [Z0, np.zeros(nc) if mu is None else mu, np.zeros(nc) if rho is None else rho, np.zeros(n) if lo is None else lo, np.zeros(n) if hi is None else hi,
              np.full(16, np.nan), np.full((outer * trials, 8), np.nan), np.full((outer, 4), np.nan), np.full(n, np.nan)]
    (dZ, dmu, drho, dlo, dhi, dinfo, dhist, dohist, des), stream = device_arrays(*arrays)
    ptr = lambda t, on=True: t.data_ptr() if on else 0
    ev.reduced_minimize_dev(ptr(dZ), SIGMA, ptr(dmu, mu is not None), ptr(drho, rho is not None), 0, ptr(dlo, lo is not None), ptr(dhi, hi is not None), outer,
                            trials, harvest, ptr(dinfo), ptr(dhist), ptr(dohist), ptr(des), stream=stream, **okw)
    import torch
    torch.cuda.synchronize()
    info = dinfo.cpu().numpy()
    passes = 0 if rho is None else int(info[1]) - int(info[0] == M.M_NOT_FINITE)
    return dict(Z=dZ.cpu().numpy(), mu=dmu.cpu().numpy() if mu is not None else None, rho=drho.cpu().numpy() if rho is not None else None, info=info,
                history=dhist.cpu().numpy()[:int(info[2])], outer_history=dohist.cpu().numpy()[:passes], states=des.cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_run(got, want, what):
    for key in ("Z", "mu", "rho", "info", "history", "outer_history", "states"):
        if want[key] is None:
            continue
        a, b = np.asarray(got[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, key, a, b)


def check_bits(name, store, family, **kw):
    c, want = case_of(name), composed(name, store, kw.get("pairs", 0), kw.get("harvest", False))
    ev = evaluator(c, store, kw.get("pairs", 0))
    try:
        repeat = kw.pop("repeat", True)
        first = one_call(ev, c, name, family, want["Z0"], want["lo"], want["hi"], **kw)
        same_run(first, want, "first call")
        if repeat:
            if kw.get("pairs", 0):
                ev.newton_pairs_clear()
            same_run(one_call(ev, c, name, family, want["Z0"], want["lo"], want["hi"], **kw), want, "repeated call")
    finally:
        ev.close()
    info = want["info"]
    print(name, f"store{store}", family, "status", info[0], "outer", info[1], "trials", info[2], "accepted", info[3], "phi", info[4], "->", info[5], "max viol",
          info[8], "->", info[9], "grew", info[10], "CG iterations", info[11])
    assert info[2] >= 3, "both banks of scalars are read and written"
    return first, want


# ----------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("family", ["host", "dev"])
@pytest.mark.parametrize("store", [0, 1])
@pytest.mark.parametrize("name", list(PLAIN))
def test_without_penalties_the_call_is_the_composed_loop_bit_for_bit(name, store, family):
    first, want = check_bits(name, store, family)
    assert 0 < want["info"][3] and want["info"][0] == M.M_MAX_TRIALS and want["info"][1] == 1 and len(want["outer_history"]) == 0
    if name == "scaled_12x9+con":
        assert want["info"][3] < want["info"][2], "a rejected trial takes part"
        assert np.any(want["states"] >= B.HELD_LO), "the box takes part"


@pytest.mark.parametrize("name,store,family", [("al_12x9", 0, "host"), ("al_12x9", 1, "dev"), ("al_8x70", 0, "dev"), ("al_8x70", 1, "host"),
                                               ("al_8x300", 0, "host"), ("al_8x300", 1, "dev")])
def test_with_penalties_the_call_is_the_composed_loop_bit_for_bit(name, store, family):
    first, want = check_bits(name, store, family, repeat=name != "al_12x9")
    outer, trials, _ = settings(name)
    assert want["info"][0] == M.M_MAX_OUTER and want["info"][1] == outer and want["info"][2] == outer * trials and len(want["outer_history"]) == outer
    n_dyn = case_of(name)["n_dyn"]
    assert np.all(first["mu"][:n_dyn] == 0.0) and np.all(first["rho"][:n_dyn] == 0.0), "the dynamics rows are untouched"
    assert np.any(first["mu"][n_dyn:] != 0.0), "mu <- mu_eff"


def test_with_a_pair_store_the_call_is_the_composed_preconditioned_loop():
    """newton_pairs = 8 and harvest: every step is the preconditioned step and its pairs feed the next; capacity 0 is the plain steps'
    run of the test above"""
    name = "al_12x9"
    over = (("outer", 2), ("trials", 4))
    c, want = case_of(name), composed(name, 0, 8, True, over)
    plain = composed(name, 0)
    ev = evaluator(c, 0, 8)
    try:
        got = one_call(ev, c, name, "host", want["Z0"], None, None, pairs=8, harvest=True, over=dict(over))
        count = ev.newton_pairs_info()[0]
    finally:
        ev.close()
    same_run(got, want, "harvest")
    print("harvested", want["info"][12], "fallbacks", want["info"][13], "CG iterations", want["info"][11], "plain steps' (8 trials)", np.sum(plain["history"][:4, 6]) +
          np.sum(plain["history"][10:14, 6]), "pairs in the store", count)
    assert want["info"][12] > 0 and count > 0, "pairs were harvested"
    assert np.array_equal(bits(want["history"][0]), bits(plain["history"][0])), "the first step has an empty store: the plain step's bits"


# --------------------------------------------------------------------------------------------------------------- oracle
def test_the_one_call_run_follows_the_oracles_outer_loop():
    """test_gpu_auglag.test_the_outer_loop_follows_the_oracles_run's bars, unchanged, on the one call"""
    c, want = case_of("al_12x9"), A.oracle_outer_run("al_12x9")
    ev = evaluator(c, 0)
    try:
        got = one_call(ev, c, "al_12x9", "host", np.array(c["Z"]), None, None)
    finally:
        ev.close()
    accepted = got["history"][:, 1].reshape(5, 10).astype(bool).tolist()
    grew, viol, viol0 = got["outer_history"][:, 1].astype(bool).tolist(), got["outer_history"][:, 0].tolist(), got["info"][8]
    print("engine: max viol", viol0, viol, "rho grew", grew)
    print("oracle: max viol", want["viol0"], want["viol"], "rho grew", want["grew"])
    assert accepted == want["accepted"] and grew == want["grew"]
    for a, b in zip(viol, want["viol"]):
        assert b / 2.0 <= a <= 2.0 * b, (a, b)
    assert viol0 >= 0.1 and viol[-1] < 1e-4 and got["info"][9] == viol[-1] and got["info"][10] == sum(grew)


def test_the_boxed_run_accepts_the_oracles_trials_and_stays_in_the_box():
    name = "scaled_12x9+con"
    c, want = case_of(name), composed(name, 0)
    o_run, (o_iterates, o_values, o_accepted), _ = M.oracle_box_run(name, 0.3)
    ev = evaluator(c, 0)
    try:
        got = one_call(ev, c, name, "host", want["Z0"], want["lo"], want["hi"])
    finally:
        ev.close()
    same_run(got, want, "boxed run")
    accepted = got["history"][:, 1].astype(bool).tolist()
    print("engine accepted", accepted, "oracle", o_accepted)
    assert accepted == o_accepted
    Cidx, lo, hi = R.index_sets(c["p"])[1], want["lo"], want["hi"]
    for Zk in want["iterates"] + [got["Z"]]:             # the composed loop's iterates are the call's, bit for bit
        assert np.all(Zk[Cidx] >= lo[Cidx]) and np.all(Zk[Cidx] <= hi[Cidx]), "inside the box, exactly"
    values = [got["info"][4]] + [row[3] for row in got["history"] if row[1]]
    assert np.all(np.diff(values) <= 0.0) and len(values) >= 2 and values[-1] == got["info"][5], "phi does not increase over the accepted trials"


# ---------------------------------------------------------------------------------------------------------------- stops
def test_the_stops():
    name = "scaled_12x9+con"
    c, base = case_of(name), composed(name, 0)
    gnorms = base["history"][:, 7]
    gtol = float(np.sort(gnorms)[len(gnorms) // 2])           # ends the inner loop at the first step whose ||g|| is no larger
    want_g = composed(name, 0, over=(("gtol", gtol),))
    want_r = composed(name, 0, over=(("radius_min", 0.3),))
    ev = evaluator(c, 0)
    try:
        ev.profile_enable(True)
        ev.auglag_merit(base["Z0"], SIGMA, c["mu"], None)
        ev.profile_reset()
        ev.auglag_merit(base["Z0"], SIGMA, c["mu"], None)
        per_merit = launches(ev, ("feasible",))[0]
        ev.profile_reset()
        got_g = one_call(ev, c, name, "host", base["Z0"], base["lo"], base["hi"], over=dict(gtol=gtol))
        merit_launches = launches(ev, ("feasible",))[0]
        ev.profile_enable(False)
        got_r = one_call(ev, c, name, "host", base["Z0"], base["lo"], base["hi"], over=dict(radius_min=0.3))
    finally:
        ev.close()
    same_run(got_g, want_g, "gtol")
    k = int(got_g["info"][2])
    print("gtol", gtol, "trials", k, "of", len(gnorms), "merits", want_g["merits"], "launches under feasible", merit_launches, "per merit", per_merit)
    assert got_g["info"][0] == M.M_CONVERGED and 1 <= k < 10 and got_g["history"][-1][1] == 0.0 and got_g["history"][-1][7] <= gtol
    assert want_g["merits"] == k and merit_launches == k * per_merit and per_merit > 0, "no merit launch behind the last step"
    same_run(got_r, want_r, "radius_min")
    assert got_r["info"][0] == M.M_RADIUS and got_r["info"][6] == 0.25 and got_r["history"][-1][0] < 0.25, "RADIUS behind the first shrink"
    assert np.all(got_r["history"][:, 2] == 1.0)


# -------------------------------------------------------------------------------------------------------- launch counts
def test_launch_counts():
    """ "minimize" counts one launch per trial and one per outer iteration; the step behind the rejected trial 1 of al_12x9 finds its kept
    points: a run of two trials makes, under the rebuild names, what a run of one trial makes plus the second trial's merit alone"""
    name = "al_12x9"
    c = case_of(name)
    full = composed(name, 0)
    assert not full["accepted"][0][0], "trial 1 is rejected"
    ev = evaluator(c, 0)
    try:
        ev.profile_enable(True)
        counts = {}
        one_call(ev, c, name, "host", np.array(c["Z"]), None, None, over=dict(outer=1, trials=1))   # every counted run starts at kept points
        for trials in (1, 2, 3):
            ev.profile_reset()
            got = one_call(ev, c, name, "host", np.array(c["Z"]), None, None, over=dict(outer=1, trials=trials))
            counts[trials] = launches(ev, REBUILD_NAMES)
            assert launches(ev, ("minimize",)) == (trials + 1,) and got["info"][2] == trials
            assert ev.profile_get("minimize")[2] > 0, "bytes"
        # the second trial's merit alone, at its own trial point
        Zf = full["iterates"][0]
        step, merit, rows = composed_callables(ev, None, None, M.options(**A.STEP_KW))
        _, Zp2, _ = step(Zf, full["history"][1][2], c["mu"], c["rho"])
        ev.profile_reset()
        merit(Zp2, c["mu"], c["rho"])
        lone = launches(ev, REBUILD_NAMES)
        ev.profile_reset()
        one_call(ev, c, name, "host", np.array(c["Z"]), None, None, over=dict(outer=2, trials=3))
        assert launches(ev, ("minimize",)) == (2 * 3 + 2,)
        ev.profile_enable(False)
    finally:
        ev.close()
    second = tuple(b - a for a, b in zip(counts[1], counts[2]))
    print("rebuild names", REBUILD_NAMES, "one trial", counts[1], "two trials", counts[2], "the second trial's merit alone", lone)
    assert second == lone, "the step behind a rejected trial makes no chain, tree-build, assembly or rollout launch"


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_device_handle_leave_nothing_enqueued_and_the_handle_usable():
    name = "al_12x9"
    c = case_of(name)
    Z, mu, rho = np.array(c["Z"]), c["mu"], c["rho"]
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)                # a sharded handle: what the composed calls refuse
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_projected_minimize.* unsharded handle"):
            ev.reduced_minimize(Z, SIGMA, mu, rho, outer=2)
    finally:
        ev.close()
    ev = evaluator(c, 0)
    try:
        ev.profile_enable(True)
        bad = np.array(rho)
        bad[c["n_dyn"] + 1] = -2.0
        for kw, word in ((dict(rho=bad), rf"rho\[{c['n_dyn'] + 1}\]"), (dict(trials=0), "trials"), (dict(outer=0), "outer"), (dict(harvest=True), "harvest"),
                         (dict(radius0=0.0), "radius0"), (dict(eta_grow=0.1), "eta_grow"), (dict(max_iter=0), "max_iter"), (dict(gtol=-1.0), "gtol")):
            with pytest.raises(dto_amd.EngineError, match=word):
                ev.reduced_minimize(Z, SIGMA, mu, **dict(dict(rho=rho, outer=2), **kw))
        with pytest.raises(dto_amd.EngineError, match="without rho"):
            ev.reduced_minimize(Z, SIGMA, mu, None, outer=2)
        assert ev.profile_get("minimize")[1] == 0 and ev.profile_get("all")[1] == 0 and ev.profile_get("feasible")[1] == 0, "nothing was enqueued"
        ev.profile_enable(False)
        want = composed(name, 0, over=(("outer", 1), ("trials", 3)))
        same_run(one_call(ev, c, name, "host", Z, None, None, over=dict(outer=1, trials=3)), want, "after the refusals")
    finally:
        ev.close()

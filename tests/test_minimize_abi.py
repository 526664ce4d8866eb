"""CPU checks of the minimize call's boundary (include/dto_engine.h, "Reduced-space minimize"): the two entry points are declared,
exported and typed alike in the header, the ctypes table and the Julia file; the option indices and the status codes agree in the
header, the plan header, capi and the Julia file; a structure-only handle, which needs no GPU, refuses with text and stays usable; and
every refusal the call states is made with text before the handle is judged, with nothing written."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import minimize_cases as M
from helpers import to_engine
from test_newton_abi import c_kind, header_source, header_text, julia_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Z, sigma, mu, rho, free_mask, lo, hi, options, outer, trials, harvest, info, history, outer_history, entry_state
KINDS = ["handle", "ptr", "double", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "int32", "int32", "int32", "ptr", "ptr", "ptr", "ptr"]
NAMES = ["dto_projected_minimize", "dto_projected_minimize_dev"]


def kinds_of(name):
    return KINDS + (["stream"] if name.endswith("_dev") else [])


def test_the_two_names_are_declared_and_typed():
    src = header_source()
    for n in NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{n} is not declared"
        assert [c_kind(a) for a in m.group(1).split(",")] == kinds_of(n), n
    assert re.search(r"#define\s+DTO_ABI_VERSION\s+8\b", src) and dto_amd.capi.DTO_ABI_VERSION == 8, "additions only: the version stays"


def test_the_ctypes_prototypes_are_typed_like_the_header():
    host = {"handle": C.c_void_p, "ptr": dto_amd.capi.c_double_p, "double": C.c_double, "int32": C.c_int32}
    dev = dict(host, ptr=C.c_void_p, stream=C.c_void_p)
    for n in NAMES:
        res, args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int
        assert list(args) == [(dev if n.endswith("_dev") else host)[k] for k in kinds_of(n)], n


def test_the_julia_file_names_both_entry_points_typed_like_the_header():
    src = julia_source()
    jl = {"handle": "Ptr{Cvoid}", "ptr": "Ptr{Float64}", "double": "Float64", "int32": "Int32", "stream": "Ptr{Cvoid}"}
    for n in NAMES:
        m = re.search(r"@ccall\s+lib\." + n + r"\((.*?)\)::Cint", src, flags=re.S)
        assert m, f"{n} has no @ccall"
        types = [a.strip().split("::")[-1] for a in m.group(1).split(",")]
        assert types == [jl[k] for k in kinds_of(n)], (n, types)
    for f in ("reduced_minimize!", "reduced_minimize_dev!", "minimize_options"):
        assert re.search(r"^(function )?" + re.escape(f) + r"\(", src, flags=re.M), f


def test_the_option_indices_and_the_status_codes_agree_everywhere():
    src, jl = header_source(), julia_source()
    plan = open(os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_minimize_plan.h")).read()
    for i, name in enumerate(M.OPTIONS):
        assert re.search(rf"#define\s+DTO_MIN_OPT_{name.upper()}\s+{i}\b", src), name
        assert re.search(rf"\bMIN_OPT_{name.upper()} = {i}\b", plan), name
    assert re.search(r"#define\s+DTO_MIN_OPTIONS\s+16\b", src) and "MINIMIZE_OPTIONS = 16" in plan
    assert dto_amd.capi.MINIMIZE_OPTIONS == M.OPTIONS and dto_amd.capi.MINIMIZE_DEFAULTS == M.DEFAULTS
    names = re.search(r"const MINIMIZE_OPTION_NAMES = \((.*?)\)", jl, flags=re.S).group(1)
    assert [w.strip().lstrip(":") for w in names.split(",")] == list(M.OPTIONS)
    defaults = re.search(r"const MINIMIZE_OPTION_DEFAULTS = \((.*?)\)", jl).group(1)
    assert [float(w.replace("Inf", "inf")) for w in defaults.split(",")] == list(M.DEFAULTS)
    codes = dict(CONVERGED=M.M_CONVERGED, MAX_OUTER=M.M_MAX_OUTER, MAX_TRIALS=M.M_MAX_TRIALS, RADIUS=M.M_RADIUS, NOT_FINITE=M.M_NOT_FINITE)
    for word, v in codes.items():
        assert re.search(rf"#define\s+DTO_MINIMIZE_{word}\s+{v}\b", src), word
        assert re.search(rf"\bMINIMIZE_{word} = {v}\b", plan), word
        assert getattr(dto_amd.capi, "MINIMIZE_" + word) == v
        assert re.search(rf"const DTO_MINIMIZE_{word} = Int32\({v}\)", jl), word


def test_the_header_section_the_plan_header_and_the_profile_name():
    text = header_text()
    a, b, c = text.index("---- Preconditioned truncated-Newton step"), text.index("---- Reduced-space minimize"), text.index("---- Multi-GPU")
    assert a < b < c
    section = text[b:c]
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", section), n
    for word in ("minimize_trial_decide", "minimize_outer_decide", "eta_accept", "radius_min", "GRADIENT", "a NaN grows the penalty", "info [16]",
                 "[outer * trials][8]", "[outer][4]", "two banks", "32-byte mailbox", "bit for bit", "Refused with text", "rounded on its own"):
        assert word in section, word
    assert '"minimize"' in text[text.index("int dto_profile_enable"):], "the profile name is listed"
    plan = open(os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_minimize_plan.h")).read()
    assert '#include "dto_newton_plan.h"' in plan and "hip" not in re.sub(r"//.*", "", plan).lower().replace("__hipcc__", "")
    assert "dto_minimize.$(O)" in open(os.path.join(ROOT, "Makefile")).read()
    kernels = open(os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_minimize.hip")).read()
    assert "k_minimize_trial" in kernels and "k_minimize_outer" in kernels and "asm" not in kernels and "atomic" not in re.sub(r"//.*", "", kernels)


def test_the_library_exports_them(engine_lib):
    lib = os.path.join(ROOT, "directtrajopt.jl_amd", "libdto_engine.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES:
        assert n in exported, f"{n} is not exported"
        assert hasattr(engine_lib, n)


@pytest.fixture()
def structure_only():
    ev = dto_amd.Evaluator(to_engine(O.make_scaled_problem(5, 6, 2, seed=4, with_constraint=True)), device=-1)
    yield ev
    ev.close()


def test_a_structure_only_handle_refuses_with_text_and_stays_usable(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    Z, mu = np.zeros(n), np.zeros(m)
    for call in (lambda: ev.reduced_minimize(Z),
                 lambda: ev.reduced_minimize(Z, 0.7, mu, np.full(m, 10.0), lo=np.full(n, -1.0), hi=np.ones(n), free=np.ones(n), outer=2, trials=3,
                                             history=True, states=True, shift=1.0, max_iter=4, gtol=1e-3),
                 lambda: ev.reduced_minimize_dev(8, 1.0, 0, 0, 0, 0, 0, 1, 5, False, 8 + 8 * n)):
        with pytest.raises(dto_amd.EngineError, match="structure-only"):
            call()
    rows, cols = ev.jacobian_structure()
    assert rows.size == ev.n_jacobian_entries == cols.size
    with pytest.raises(ValueError, match="wrong length"):
        ev.reduced_minimize(Z[:-1])
    for word in ("free", "lo", "hi", "mu", "rho"):
        with pytest.raises(ValueError, match=word):
            ev.reduced_minimize(Z, **dict(dict(mu=mu) if word == "rho" else {}, **{word: np.ones(3)}))
    with pytest.raises(TypeError, match="unknown option"):
        ev.reduced_minimize(Z, radius=1.0)


BAD = [
    (dict(outer=0), "outer = 0"), (dict(trials=0), "trials = 0"), (dict(trials=-2), "trials = -2"), (dict(outer=2), "outer = 2 without rho"),
    (dict(rho=True, mu=None, outer=2), "mu is NULL"),
    (dict(radius0=0.0), "radius0"), (dict(radius0=-1.0), "radius0"), (dict(radius0=np.inf), "radius0"), (dict(radius0=np.nan), "radius0"),
    (dict(eta_accept=-0.1), "eta_accept"), (dict(gtol=np.nan), "gtol"), (dict(ctol=-1.0), "ctol"), (dict(radius_min=-1.0), "radius_min"),
    (dict(radius_max=np.nan), "radius_max"), (dict(viol_div=-4.0), "viol_div"), (dict(rho_mul=np.nan), "rho_mul"), (dict(shift=-1.0), "shift"),
    (dict(eta_accept=0.3), "eta_accept <= eta_shrink < eta_grow"), (dict(eta_shrink=0.75), "eta_accept <= eta_shrink < eta_grow"),
    (dict(eta_grow=0.2), "eta_accept <= eta_shrink < eta_grow"),
    (dict(shrink_div=1.0), "shrink_div"), (dict(grow_mul=0.5), "grow_mul"),
    (dict(max_iter=0), "max_iter"), (dict(max_iter=2.5), "max_iter"), (dict(rtol=np.inf), "rtol"), (dict(atol=np.inf), "atol"), (dict(shift=np.inf), "shift"),
    (dict(harvest=True), "harvest needs a pair store"),
]


@pytest.mark.parametrize("kw,word", BAD, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in BAD])
def test_every_refusal_is_made_with_text_before_the_handle_is_judged(structure_only, kw, word):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    kw = dict(kw)
    if kw.pop("rho", False):
        kw["rho"] = np.full(m, 10.0)
    with pytest.raises(dto_amd.EngineError, match=word) as e:
        ev.reduced_minimize(np.zeros(n), **kw)
    assert "structure-only" not in str(e.value) and "dto_projected_minimize" in str(e.value)
    dev = dict(outer=kw.pop("outer", 1), trials=kw.pop("trials", 5), harvest=kw.pop("harvest", False))
    drho = 8 + 16 * n if "rho" in kw else 0
    kw.pop("rho", None), kw.pop("mu", None)
    with pytest.raises(dto_amd.EngineError, match=word) as e:
        ev.reduced_minimize_dev(8, 1.0, 0, drho, 0, 0, 0, dev["outer"], dev["trials"], dev["harvest"], 8 + 8 * n, **kw)
    assert "structure-only" not in str(e.value) and "dto_projected_minimize_dev" in str(e.value)


def test_a_bad_penalty_is_refused_naming_the_row(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    rho = np.full(m, 1.0)
    rho[m - 1] = -2.0
    with pytest.raises(dto_amd.EngineError, match=rf"dto_projected_minimize: rho\[{m - 1}\]") as e:
        ev.reduced_minimize(np.zeros(n), 1.0, np.zeros(m), rho)
    assert "structure-only" not in str(e.value)


def _call(ev, Z, info, mu=None, rho=None, mask=None, lo=None, hi=None, hist=None, ohist=None, es=None, outer=1, trials=2):
    dp = lambda a: None if a is None else a.ctypes.data_as(dto_amd.capi.c_double_p)
    rc = ev._lib.dto_projected_minimize(ev._h, dp(Z), 1.0, dp(mu), dp(rho), dp(mask), dp(lo), dp(hi), None, outer, trials, 0, dp(info), dp(hist), dp(ohist),
                                      dp(es))
    return rc, ev._lib.dto_last_error(ev._h).decode()


def test_null_pointers_and_overlapping_outputs_are_refused_with_text(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    for z_, i_ in ((None, np.zeros(16)), (np.zeros(n), None)):
        rc, text = _call(ev, z_, i_)
        assert rc != 0 and "NULL" in text and "dto_projected_minimize" in text
    pool = np.zeros(8 * n + 2 * m + 16 + 16 + 4)
    part = lambda k: pool[k * n:(k + 1) * n]
    Z, mask, lo, hi, es = (part(k) for k in range(5))
    mu, rho = pool[8 * n:8 * n + m], pool[8 * n + m:8 * n + 2 * m]
    rho[:] = 1.0
    info, hist, ohist = pool[8 * n + 2 * m:][:16], pool[8 * n + 2 * m + 16:][:16], pool[8 * n + 2 * m + 32:][:4]
    good = dict(Z=Z, info=info, mu=mu, rho=rho, mask=mask, lo=lo, hi=hi, hist=hist, ohist=ohist, es=es)
    label = dict(Z="Z", es="entry_state", info="info", hist="history", ohist="outer_history", mu="mu", rho="rho", mask="free_mask", lo="lo", hi="hi")
    for out_name in ("Z", "es"):                                   # an output against every input: the whole vector, and its last entry
        for in_name in ("mask", "lo", "hi"):
            k = ("Z", "mask", "lo", "hi").index(in_name)
            for alias in (part(k), pool[k * n + n - 1:][:n]):
                rc, text = _call(ev, **dict(good, **{out_name: alias}))
                assert rc != 0 and f"{label[out_name]} overlaps {label[in_name]}" in text and "structure-only" not in text, (out_name, in_name, text)
    for a, b in (("Z", "es"), ("mu", "rho"), ("info", "hist"), ("hist", "ohist"), ("Z", "info")):      # outputs against each other
        rc, text = _call(ev, **dict(good, **{b: good[a][:good[b].size] if good[a].size >= good[b].size else good[a]}))
        assert rc != 0 and f"{label[a]} overlaps {label[b]}" in text and "structure-only" not in text, (a, b, text)
    before = pool.copy()
    rc, text = _call(ev, **good)
    assert rc != 0 and "structure-only" in text, "disjoint buffers: the handle is judged next"
    assert np.array_equal(pool, before), "nothing was written"
    assert ev.jacobian_structure()[0].size == ev.n_jacobian_entries


def test_the_docstrings_exist():
    E = dto_amd.Evaluator
    for f in (E.reduced_minimize, E.reduced_minimize_dev):
        assert f.__doc__ and len(f.__doc__) > 60, f.__name__

"""CPU checks of the bound-constrained truncated-Newton boundary (include/dto_engine.h, "Bound-constrained truncated-Newton step"): the
two entry points are declared, exported and typed alike in the header, the ctypes table and the Julia file; the entry-state constants are
equal in all three; a structure-only handle, which needs no GPU, refuses with text and stays usable; every bad argument and every
overlap is refused with text naming it; and the bounds helper of the problem mirror expands per-component bounds in the trajectory's
layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine
from test_newton_abi import BAD, c_kind, header_source, header_text, julia_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dto_projected_newton_step_box", "dto_projected_newton_step_box_dev"]
# handle, Z, sigma, mu, free_mask, lo, hi, radius, shift, rtol, atol, max_iter, p, info, trace, entry_state, Zp (, stream)
KINDS = ["handle", "ptr", "double", "ptr", "ptr", "ptr", "ptr", "double", "double", "double", "double", "int32", "ptr", "ptr", "ptr", "ptr", "ptr"]
STATES = {"FIXED": 0, "FREE": 1, "HELD_LOWER": 2, "HELD_UPPER": 3, "HIT_LOWER": 4, "HIT_UPPER": 5}


def kinds_of(name):
    return KINDS + (["stream"] if name.endswith("_dev") else [])


def test_the_two_names_are_declared_and_typed():
    src = header_source()
    for n in NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{n} is not declared"
        assert [c_kind(a) for a in m.group(1).split(",")] == kinds_of(n), n
    assert re.search(r"#define\s+DTO_ABI_VERSION\s+8\b", src) and dto_amd.capi.DTO_ABI_VERSION == 8, "an addition: the version stays"


def test_the_ctypes_prototypes_are_typed_like_the_header():
    host = {"handle": C.c_void_p, "ptr": dto_amd.capi.c_double_p, "double": C.c_double, "int32": C.c_int32}
    dev = dict(host, ptr=C.c_void_p, stream=C.c_void_p)
    for n in NAMES:
        res, args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int
        table = dev if n.endswith("_dev") else host
        assert list(args) == [table[k] for k in kinds_of(n)], n


def test_the_julia_file_names_both_entry_points_typed_like_the_header():
    src = julia_source()
    jl = {"handle": "Ptr{Cvoid}", "ptr": "Ptr{Float64}", "double": "Float64", "int32": "Int32", "stream": "Ptr{Cvoid}"}
    for n in NAMES:
        m = re.search(r"@ccall\s+lib\." + n + r"\((.*?)\)::Cint", src, flags=re.S)
        assert m, f"{n} has no @ccall"
        types = [a.strip().split("::")[-1] for a in m.group(1).split(",")]
        assert types == [jl[k] for k in kinds_of(n)], (n, types)


def test_the_state_constants_are_equal_in_all_three():
    defs = dict(re.findall(r"#define (DTO_BOX_\w+) (\d+)", header_source()))
    consts = dict(re.findall(r"const (DTO_BOX_\w+) = Int32\((\d+)\)", julia_source()))
    assert set(defs) == set(consts) == {"DTO_BOX_" + k for k in STATES}
    for k, v in STATES.items():
        assert int(defs["DTO_BOX_" + k]) == int(consts["DTO_BOX_" + k]) == getattr(dto_amd.capi, "BOX_" + k) == v, k


def test_the_header_section_the_plan_header_and_the_profile_name():
    text = header_text()
    a, b, c = text.index("---- Truncated-Newton step"), text.index("---- Bound-constrained truncated-Newton step"), text.index("---- Multi-GPU")
    assert a < b < c
    section = text[b:c]
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", section), n
    for word in ("tau_box", "restart", "n_hit", "state 5", "state 4", "newton_box_decide", "Refused with text", "rounded on its own", "EXACTLY",
                 "info [12]", "[max_iter][6]", "bit for bit"):
        assert word in section, word
    assert '"newton_box"' in text[text.index("int dto_profile_enable"):]
    plan = open(os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_newton_box_plan.h")).read()
    assert '#include "dto_newton_plan.h"' in plan and "hip" not in re.sub(r"//.*", "", plan).lower().replace("__hipcc__", "")
    assert "dto_newton_box.$(O)" in open(os.path.join(ROOT, "Makefile")).read()


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
    n = ev.n_variables
    Z, mu = np.zeros(n), np.zeros(ev.n_constraints)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_newton_step_box(Z)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_newton_step_box(Z, 0.7, mu, lo=np.full(n, -1.0), hi=np.ones(n), free=np.ones(n), radius=1.0, shift=2.0, max_iter=3, trace=True,
                                   states=True, trajectory=True)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_newton_step_box_dev(8, 1.0, 0, 0, 0, 0, 0.0, 0.0, 1e-6, 0.0, 5, 8 + 8 * n, 8 + 16 * n)
    rows, cols = ev.jacobian_structure()
    assert rows.size == ev.n_jacobian_entries == cols.size
    with pytest.raises(ValueError, match="wrong length"):
        ev.reduced_newton_step_box(Z[:-1])
    for word in ("free", "lo", "hi"):
        with pytest.raises(ValueError, match=word):
            ev.reduced_newton_step_box(Z, **{word: np.ones(3)})


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD])
def test_what_the_unbounded_step_refuses_is_refused_with_text(structure_only, kw, word):
    """the arguments are judged before the handle is: a structure-only handle names the bad one (a good call says "structure-only")"""
    ev = structure_only
    n = ev.n_variables
    Z = np.zeros(n)
    with pytest.raises(dto_amd.EngineError, match=word) as e:
        ev.reduced_newton_step_box(Z, lo=np.full(n, -1.0), **kw)
    assert "structure-only" not in str(e.value) and "dto_projected_newton_step_box" in str(e.value)
    with pytest.raises(dto_amd.EngineError, match=word):
        ev.reduced_newton_step_box_dev(8, 1.0, 0, 0, 0, 0, kw.get("radius", 0.0), kw.get("shift", 0.0), kw.get("rtol", 1e-6), kw.get("atol", 0.0),
                                       kw.get("max_iter", 5), 8 + 8 * n, 8 + 16 * n)


def _call(ev, Z, p, info, mask=None, lo=None, hi=None, trace=None, es=None, zp=None):
    dp = lambda a: None if a is None else a.ctypes.data_as(dto_amd.capi.c_double_p)
    rc = ev._lib.dto_projected_newton_step_box(ev._h, dp(Z), 1.0, None, dp(mask), dp(lo), dp(hi), 0.0, 0.0, 1e-6, 0.0, 5, dp(p), dp(info), dp(trace),
                                               dp(es), dp(zp))
    return rc, ev._lib.dto_last_error(ev._h).decode()


def test_null_pointers_are_refused_with_text(structure_only):
    ev = structure_only
    n = ev.n_variables
    Z, p, info = np.zeros(n), np.full(n, np.nan), np.full(12, np.nan)
    for z_, p_, i_ in ((None, p, info), (Z, None, info), (Z, p, None)):
        rc, text = _call(ev, z_, p_, i_)
        assert rc != 0 and "NULL" in text and "dto_projected_newton_step_box" in text
    for z_, p_, i_ in ((None, 8, 8), (8, None, 8), (8, 8, None)):
        assert ev._lib.dto_projected_newton_step_box_dev(ev._h, z_, 1.0, None, None, None, None, 0.0, 0.0, 1e-6, 0.0, 5, p_, i_, None, None, None,
                                                         None) != 0
        assert "NULL" in ev._lib.dto_last_error(ev._h).decode()
    assert np.isnan(p).all() and np.isnan(info).all()
    assert ev.jacobian_structure()[0].size == ev.n_jacobian_entries


def test_overlapping_outputs_are_refused_with_text(structure_only):
    """p, Zp and entry_state against Z, the mask and the bounds: twelve pairs, each named; a partial overlap counts"""
    ev = structure_only
    n = ev.n_variables
    info = np.full(12, np.nan)
    pool = np.zeros(8 * n)
    part = lambda k: pool[k * n:(k + 1) * n]
    Z, mask, lo, hi, p, es, zp = (part(k) for k in range(7))
    ins = dict(Z=Z, free_mask=mask, lo=lo, hi=hi)
    for out_name in ("p", "Zp", "entry_state"):
        for k, in_name in enumerate(("Z", "free_mask", "lo", "hi")):
            for alias in (part(k), pool[k * n + n - 1:][:n]):       # the whole vector, and its last entry alone
                outs = dict(p=p, Zp=zp, entry_state=es)
                outs[out_name] = alias
                rc, text = _call(ev, Z, outs["p"], info, mask=mask, lo=lo, hi=hi, es=outs["entry_state"], zp=outs["Zp"])
                assert rc != 0 and f"{out_name} overlaps {in_name}" in text, (out_name, in_name, text)
                assert "structure-only" not in text
    rc, text = _call(ev, Z, p, info, mask=mask, lo=lo, hi=hi, es=es, zp=zp)
    assert rc != 0 and "structure-only" in text, "disjoint buffers: the handle is judged next"
    assert np.isnan(info).all() and not pool.any(), "nothing was written"
    dev = ev._lib.dto_projected_newton_step_box_dev
    base = 1 << 20
    assert dev(ev._h, base, 1.0, None, None, base + 8 * n, None, 0.0, 0.0, 1e-6, 0.0, 5, base + 16 * n, 8, None, None, base + 8 * (2 * n - 1), None) != 0
    assert "Zp overlaps lo" in ev._lib.dto_last_error(ev._h).decode()


def test_the_docstrings_exist():
    E = dto_amd.Evaluator
    for f in (E.reduced_newton_step_box, E.reduced_newton_step_box_dev, dto_amd.DirectTrajOptProblem.bounds_vectors):
        assert f.__doc__ and len(f.__doc__) > 80, f.__name__


# ------------------------------------------------------------------------------------------------------- the bounds helper
def two_component_problem():
    N = 4
    traj = dto_amd.NamedTrajectory({"x": np.zeros((3, N)), "u": np.zeros((2, N)), "dt": np.full((1, N), 0.1)}, timestep="dt",
                                   global_data=np.zeros(2), global_components={"g": [0, 1]})
    return dto_amd.DirectTrajOptProblem(traj, dto_amd.NullObjective(traj), []), traj


def test_the_bounds_helper_follows_the_component_layout():
    prob, traj = two_component_problem()
    N, dim = traj.N, traj.dim
    assert dim == 6 and list(traj.components["u"]) == [3, 4] and list(traj.components["dt"]) == [5]
    lo, hi = prob.bounds_vectors({"u": (-1.0, [0.5, 2.0]), "dt": (0.01, None), "g": ([-3.0, -4.0], 7.0)})
    assert lo.shape == hi.shape == (N * dim + 2,)
    L, Hh = lo[:N * dim].reshape(N, dim), hi[:N * dim].reshape(N, dim)
    assert np.all(L[:, :3] == -np.inf) and np.all(Hh[:, :3] == np.inf), "x has no bound"
    assert np.all(L[:, 3:5] == -1.0) and np.all(Hh[:, 3] == 0.5) and np.all(Hh[:, 4] == 2.0), "a scalar and a per-row vector, at every knot"
    assert np.all(L[:, 5] == 0.01) and np.all(Hh[:, 5] == np.inf), "None: no bound on that side"
    assert np.array_equal(lo[N * dim:], [-3.0, -4.0]) and np.array_equal(hi[N * dim:], [7.0, 7.0]), "global components lie behind the last knot"
    lo2, hi2 = prob.bounds_vectors({})
    assert np.all(lo2 == -np.inf) and np.all(hi2 == np.inf)
    with pytest.raises(KeyError, match="no component"):
        prob.bounds_vectors({"v": (0.0, 1.0)})
    with pytest.raises(ValueError, match="rows"):
        prob.bounds_vectors({"u": ([0.0, 0.0, 0.0], 1.0)})
    with pytest.raises(ValueError, match="pair"):
        prob.bounds_vectors({"u": (0.0,)})

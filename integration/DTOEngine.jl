# DTOEngine.jl -- the reference-side binding of libdto_engine.so (include/dto_engine.h, ABI version 8).
#
# Drop this file into DirectTrajOpt.jl (e.g. src/solvers/DTOEngine.jl, `include`d from src/solvers/_solvers.jl) and
# replace the evaluator at the two swap points:
#
#     src/solvers/ipopt_solver/solver.jl:68-69   evaluator = DTOEngine.GPUEvaluator(prob; eval_hessian = options.eval_hessian)
#     ext/MadNLPSolverExt/solver.jl:81           evaluator = DTOEngine.GPUEvaluator(prob; eval_hessian = true)
#
# `GPUEvaluator <: MOI.AbstractNLPEvaluator` implements the same MOI methods as `Solvers.Evaluator`
# (src/solvers/evaluator.jl:291-456) and carries the fields other code reads off it (`trajectory`, `n_constraints`,
# `n_dynamics_constraints`, `n_nonlinear_constraints`, evaluator.jl:66-98).  Everything the engine implements natively
# runs on the GPU: BilinearIntegrator, DerivativeIntegrator, QuadraticRegularizer, LinearRegularizer,
# MinimumTimeObjective, CompositeObjective.  Terms that are Julia closures (KnotPointObjective, NonlinearKnotPoint-
# Constraint, TimeDependentBilinearIntegrator and other integrators, GlobalObjective, GlobalKnotPointObjective,
# NonlinearGlobalConstraint) are evaluated HERE with the reference's own functions (`evaluate!`, `eval_jacobian`,
# `eval_hessian_of_lagrangian`, `objective_value`, `gradient!`, `get_full_hessian`, or ForwardDiff on the closure exactly as
# those functions do) and merged by the engine at its precomputed offsets (`dto_set_external`).
#
# Beyond the MOI surface the file binds the device-resident entry points (`*_dev!`: MadNLP GPU mode,
# src/solvers/madnlp_solver/options.jl:12-16 -- value vectors never cross PCIe) and the engine's multi-GPU collectives
# (`comm_create!`, `gather_jacobian_dev!` and friends: RCCL over xGMI behind the C ABI).
#
# This file cannot be executed in the build environment of the engine (no Julia there); tests/test_julia_shim.py checks
# its struct layouts and ccall signatures against include/dto_engine.h.
module DTOEngine

using LinearAlgebra
using SparseArrays
using ForwardDiff
import MathOptInterface as MOI
using NamedTrajectories
using TrajectoryIndexingUtils: slice
using ..Problems: DirectTrajOptProblem
using ..Integrators: AbstractIntegrator, BilinearIntegrator, DerivativeIntegrator
using ..Objectives: AbstractObjective, CompositeObjective, NullObjective, QuadraticRegularizer, LinearRegularizer,
    MinimumTimeObjective, GlobalObjective, GlobalKnotPointObjective, objective_value, gradient!, get_full_hessian
using ..Constraints: AbstractNonlinearConstraint, NonlinearKnotPointConstraint, NonlinearGlobalConstraint
using ..CommonInterface: evaluate!, eval_jacobian, eval_hessian_of_lagrangian

const lib = get(ENV, "DTO_ENGINE_LIB", "libdto_engine.so")
const DTO_ABI_VERSION = Int32(8)

const DTO_FLAG_BLOCK_GENERATORS = Int32(2)
const DTO_FLAG_SHARED_GENERATORS = Int32(4)  # integrators of one system: bilinear ones share the propagator chain, time-dependent ones one propagation per call
const DTO_INTEGRATOR_BILINEAR = Int32(1)
const DTO_INTEGRATOR_DERIVATIVE = Int32(2)
const DTO_INTEGRATOR_EXTERNAL = Int32(3)
const DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR = Int32(4)
const DTO_OBJECTIVE_QUADRATIC_REGULARIZER = Int32(1)
const DTO_OBJECTIVE_LINEAR_REGULARIZER = Int32(2)
const DTO_OBJECTIVE_MINIMUM_TIME = Int32(3)
const DTO_OBJECTIVE_EXTERNAL_KNOT = Int32(5)
const DTO_OBJECTIVE_EXTERNAL_GLOBAL = Int32(7)
const DTO_CONSTRAINT_EXTERNAL = Int32(3)
const DTO_CONSTRAINT_EXTERNAL_GLOBAL = Int32(4)
const DTO_CONSTRAINT_QUADFORM_MINUS_C = Int32(5)
const DTO_COMM_ID_BYTES = Int32(128)
const DTO_VECTOR_JACOBIAN = Int32(1)
const DTO_VECTOR_HESSIAN = Int32(2)
const DTO_VECTOR_GRADIENT = Int32(3)
const DTO_VECTOR_CONSTRAINT = Int32(4)
const DTO_ROLLOUT_ALL = Int32(0)    # rollout: the states of every knot, x_dim x n_cols x N
const DTO_ROLLOUT_FINAL = Int32(1)  # rollout: the states of knot N alone, x_dim x n_cols
const DTO_SOLVE_FORWARD = Int32(0)  # dynamics_solve: Y_{k+1} = E_k Y_k + B_{k+1}
const DTO_SOLVE_ADJOINT = Int32(1)  # dynamics_solve: Λ_k = E_k' Λ_{k+1} + B_k
const DTO_NEWTON_CONVERGED = Int32(0)      # newton_step: status in info[1]
const DTO_NEWTON_BOUNDARY = Int32(1)
const DTO_NEWTON_NEG_CURVATURE = Int32(2)
const DTO_NEWTON_MAX_ITER = Int32(3)
const DTO_NEWTON_NOT_FINITE = Int32(4)

# ---- plain-C structs, field for field as in include/dto_engine.h ----------------------------------------------------
struct IntegratorDesc
    kind::Int32
    x_off::Int32
    x_dim::Int32
    u_off::Int32
    u_dim::Int32
    G::Ptr{Float64}
    t_off::Int32
    spline_order::Int32
    substeps::Int32
    n_mod::Int32
    mod_kind::Ptr{Int32}
    mod_omega::Ptr{Float64}
    H::Ptr{Float64}
end
# bilinear / derivative / host-evaluated integrators leave the time-dependent fields empty
IntegratorDesc(kind, x_off, x_dim, u_off, u_dim, G) =
    IntegratorDesc(kind, x_off, x_dim, u_off, u_dim, G, Int32(0), Int32(0), Int32(0), Int32(0), Ptr{Int32}(C_NULL),
                   Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL))

struct ObjectiveDesc
    kind::Int32
    comp_off::Int32
    comp_dim::Int32
    reserved::Int32
    weight::Float64
    D::Float64
    R::Ptr{Float64}
    baseline::Ptr{Float64}
    times::Ptr{Int64}
    n_times::Int64
    comps::Ptr{Int32}
    n_comps::Int32
    reserved2::Int32
    params::Ptr{Float64}
    Qs::Ptr{Float64}
    gcomps::Ptr{Int32}
    n_gcomps::Int32
    reserved3::Int32
end

struct ConstraintDesc
    kind::Int32
    equality::Int32
    n_comps::Int32
    g_dim::Int32
    comps::Ptr{Int32}
    c::Float64
    times::Ptr{Int64}
    n_times::Int64
    jac0::Ptr{Float64}
    hess0::Ptr{Float64}
end

struct ProblemDesc
    abi_version::Int32
    device::Int32
    N::Int64
    z::Int32
    gd::Int32
    dt_idx::Int32
    eval_hessian::Int32
    n_integrators::Int32
    n_objectives::Int32
    n_constraints::Int32
    flags::Int32
    integrators::Ptr{IntegratorDesc}
    objectives::Ptr{ObjectiveDesc}
    constraints::Ptr{ConstraintDesc}
    Z0::Ptr{Float64}
    k_lo::Int64
    k_hi::Int64
end

struct ExternalValues
    values::Ptr{Float64}
    first::Ptr{Float64}
    second::Ptr{Float64}
end

struct GatherLayout
    total::Int64
    padded_len::Int64
    front_pad::Int64
    own_lo::Int64
    own_len::Int64
    in_place_all_gather::Int32
    world::Int32
end

# ---- TimeDependentBilinearIntegrator on the device ------------------------------------------------------------------
"""
The generator family the engine integrates on the GPU (DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR):

    G(u, t) = sum_{j=0..m} ubar_j ( G[:, :, j+1] + sum_c phi_c(t) H[:, :, j+1, c] ),  ubar_0 = 1,  phi_c = cos | sin (omegas[c] t)

The object is callable, so it is also the `G` the reference's constructor takes:

    fam = DTOEngine.ModulatedGenerators(G, Int32[1], [1.7], H; substeps = 32)
    B = TimeDependentBilinearIntegrator(fam, :x, :u, :t, traj; spline_order = 1)
    DTOEngine.device_family!(B, fam)        # tells the evaluator to run B on the device

(`G` is captured inside the ODE problem the integrator builds, out of reach of the struct's fields, hence the registration.)
The engine integrates with classical RK4, `substeps` fixed steps per interval, and returns the exact derivatives of that
scheme; the reference integrates adaptively (Tsit5).  Any other closure keeps running in Julia and is merged.
"""
struct ModulatedGenerators
    G::Array{Float64,3}
    kinds::Vector{Int32}      # 1 = cos, 2 = sin
    omegas::Vector{Float64}
    H::Array{Float64,4}       # n x n x (m+1) x n_mod
    substeps::Int
end
ModulatedGenerators(G, kinds, omegas, H; substeps::Int = 32) =
    ModulatedGenerators(Array{Float64,3}(G), Vector{Int32}(kinds), Vector{Float64}(omegas), Array{Float64,4}(H), substeps)
function (g::ModulatedGenerators)(u, t)
    ub = vcat(1.0, u)
    M = sum(ub[j] .* g.G[:, :, j] for j in eachindex(ub))
    for c in eachindex(g.omegas)
        phi = g.kinds[c] == 1 ? cos(g.omegas[c] * t) : sin(g.omegas[c] * t)
        M = M .+ phi .* sum(ub[j] .* g.H[:, :, j, c] for j in eachindex(ub))
    end
    return M
end
const DEVICE_FAMILIES = IdDict{Any,ModulatedGenerators}()
device_family!(B, fam::ModulatedGenerators) = (DEVICE_FAMILIES[B] = fam; B)

# ---- the evaluator --------------------------------------------------------------------------------------------------
"""
    QuadraticFormKnotConstraint(M, c, names, traj; times=[traj.N], equality=false)

g(v) = [v' M v - c] on v = z_t[names] with a constant symmetric `M`: the built-in device form (DTO_CONSTRAINT_QUADFORM_MINUS_C) of
`NonlinearKnotPointConstraint(v -> [v' * M * v - c], names, traj; times, equality)`, which as a closure is evaluated on the host
and uploaded before every callback.  `fidelity_constraint(A, names, traj, F_min)` is the final-fidelity bound of the
minimum-time stage, `NonlinearKnotPointConstraint(x -> [F_min - F(x)], names, traj; times=[N], equality=false)` with F(v) = ||A v||^2.
"""
struct QuadraticFormKnotConstraint <: AbstractNonlinearConstraint
    M::Matrix{Float64}
    c::Float64
    var_names::Vector{Symbol}
    times::Vector{Int}
    equality::Bool
    g_dim::Int
    dim::Int
    function QuadraticFormKnotConstraint(M::AbstractMatrix, c::Real, names, traj::NamedTrajectory; times=[traj.N], equality::Bool=false)
        names = names isa Symbol ? [names] : collect(Symbol, names)
        n = sum(length(traj.components[nm]) for nm in names)
        size(M) == (n, n) && M == M' || error("QuadraticFormKnotConstraint: M must be a symmetric $n x $n matrix")
        new(Matrix{Float64}(M), Float64(c), names, collect(Int, times), equality, 1, length(times))
    end
end

function fidelity_constraint(A::AbstractMatrix, names, traj::NamedTrajectory, fidelity::Real; times=[traj.N])
    M = -Matrix{Float64}(A' * A)
    QuadraticFormKnotConstraint((M + M') / 2, -fidelity, names, traj; times=times, equality=false)
end

mutable struct GPUEvaluator <: MOI.AbstractNLPEvaluator
    handle::Ptr{Cvoid}
    trajectory::NamedTrajectory
    n_variables::Int
    n_constraints::Int
    n_dynamics_constraints::Int
    n_nonlinear_constraints::Int
    eval_hessian::Bool
    jacobian_structure::Vector{Tuple{Int,Int}}
    hessian_structure::Vector{Tuple{Int,Int}}
    # host-evaluated terms, in the engine's slot order: integrators, constraints, objectives
    ext_integrators::Vector{Tuple{AbstractIntegrator,Int}}          # (integrator, first NLP row, 1-based)
    ext_constraints::Vector{Tuple{AbstractNonlinearConstraint,Int}}  # (constraint, first NLP row, 1-based)
    ext_objectives::Vector{AbstractObjective}
    ext_comps::Dict{Any,Vector{Int}}                                  # term -> knot-local component indices (1-based)
    ext_gcomps::Dict{Any,Vector{Int}}                                 # Global* term -> indices into global_data (1-based)
    staging::Vector{Vector{Float64}}                                  # keeps the blocks alive across the ccall
end

function check(ev::GPUEvaluator, rc::Integer)
    rc == 0 && return nothing
    error(unsafe_string(@ccall lib.dto_last_error(ev.handle::Ptr{Cvoid})::Cstring))
end

"""
Generators of a `BilinearIntegrator`: the struct stores only the closure `f`, which captured the user's `G`
(src/integrators/bilinear_integrator.jl:61-81), so `B.f.G` is that function.  `G` must be affine in `u`:
`G(u) = G_0 + sum_j u_j G_j`; the engine takes `G_0 = G(0)` and `G_j = G(e_j) - G(0)`.
"""
function generators(B::BilinearIntegrator, traj::NamedTrajectory)
    G = B.f.G
    m = traj.dims[B.u_name]
    G0 = Matrix{Float64}(G(zeros(m)))
    Gs = [Matrix{Float64}(G(Float64.(1:m .== j))) .- G0 for j = 1:m]
    u = randn(m)
    Gu = G0 + sum(u[j] .* Gs[j] for j = 1:m; init = zeros(size(G0)))
    isapprox(Matrix{Float64}(G(u)), Gu; rtol = 1e-12, atol = 1e-12) ||
        error("DTOEngine: G(u) of the BilinearIntegrator on :$(B.x_name) is not affine in u; keep Solvers.Evaluator for it")
    return cat(G0, Gs...; dims = 3)   # n x n x (m+1), column-major = the ABI layout
end

flatten(obj::NullObjective) = Tuple{AbstractObjective,Float64}[]
flatten(obj::AbstractObjective) = Tuple{AbstractObjective,Float64}[(obj, 1.0)]
function flatten(obj::CompositeObjective)
    out = Tuple{AbstractObjective,Float64}[]
    for (o, w) in zip(obj.objectives, obj.weights)
        o isa NullObjective && continue
        o isa CompositeObjective && error("DTOEngine: nested CompositeObjective (the reference's `+` flattens them)")
        push!(out, (o, w))
    end
    return out
end

first0(traj, name) = Int32(first(traj.components[name]) - 1)   # 0-based offset of a component inside a knot

function GPUEvaluator(prob::DirectTrajOptProblem; eval_hessian::Bool = true, device::Integer = 0, k_lo::Integer = 0, k_hi::Integer = 0,
                      block_generators::Bool = false, shared_generators::Bool = false)
    traj = prob.trajectory
    traj.timestep isa Symbol || error("DTOEngine: the engine needs a timestep component (bilinear_integrator.jl:123)")
    keep = Any[]   # everything the descriptors point at, alive until dto_create returns

    # integrators, in list order (their rows stack in that order, evaluator.jl:213-217)
    idescs = IntegratorDesc[]
    ext_integrators = Tuple{AbstractIntegrator,Int}[]
    row = 1
    for integ in prob.integrators
        if integ isa BilinearIntegrator
            G = generators(integ, traj)
            push!(keep, G)
            push!(idescs, IntegratorDesc(DTO_INTEGRATOR_BILINEAR, first0(traj, integ.x_name), Int32(integ.x_dim),
                                         first0(traj, integ.u_name), Int32(traj.dims[integ.u_name]), pointer(G)))
        elseif integ isa DerivativeIntegrator
            push!(idescs, IntegratorDesc(DTO_INTEGRATOR_DERIVATIVE, first0(traj, integ.x_name), Int32(integ.x_dim),
                                         first0(traj, integ.ẋ_name), Int32(integ.x_dim), Ptr{Float64}(C_NULL)))
        elseif haskey(DEVICE_FAMILIES, integ)   # TimeDependentBilinearIntegrator with a registered generator family
            fam = DEVICE_FAMILIES[integ]
            push!(keep, fam)
            push!(idescs, IntegratorDesc(DTO_INTEGRATOR_TIME_DEPENDENT_BILINEAR, first0(traj, integ.x_name), Int32(integ.x_dim),
                                         first0(traj, integ.u_name), Int32(integ.u_dim), pointer(fam.G),
                                         first0(traj, integ.t_name), Int32(integ.spline_order), Int32(fam.substeps),
                                         Int32(length(fam.omegas)), pointer(fam.kinds), pointer(fam.omegas), pointer(fam.H)))
        else   # TimeDependentBilinearIntegrator with an arbitrary closure, user integrators: evaluated here, merged by the engine
            push!(idescs, IntegratorDesc(DTO_INTEGRATOR_EXTERNAL, Int32(0), Int32(integ.x_dim), Int32(0), Int32(0), Ptr{Float64}(C_NULL)))
            push!(ext_integrators, (integ, row))
        end
        row += integ.dim
    end
    n_dyn = row - 1

    # objective terms (CompositeObjective flattened with its weights, _objectives.jl:106-156)
    odescs = ObjectiveDesc[]
    ext_objectives = AbstractObjective[]
    ext_comps = Dict{Any,Vector{Int}}()
    ext_gcomps = Dict{Any,Vector{Int}}()
    null = Ptr{Float64}(C_NULL)
    for (o, w) in flatten(prob.objective)
        if o isa QuadraticRegularizer || o isa LinearRegularizer
            R = Vector{Float64}(o.R)
            times = Vector{Int64}(o.times)
            base = o isa QuadraticRegularizer ? Matrix{Float64}(o.baseline) : zeros(0, 0)
            push!(keep, R, times, base)
            push!(odescs, ObjectiveDesc(o isa QuadraticRegularizer ? DTO_OBJECTIVE_QUADRATIC_REGULARIZER : DTO_OBJECTIVE_LINEAR_REGULARIZER,
                                        first0(traj, o.name), Int32(traj.dims[o.name]), Int32(0), w, 0.0, pointer(R),
                                        o isa QuadraticRegularizer ? pointer(base) : null, pointer(times), length(times),
                                        Ptr{Int32}(C_NULL), Int32(0), Int32(0), null, null, Ptr{Int32}(C_NULL), Int32(0), Int32(0)))
        elseif o isa MinimumTimeObjective
            push!(odescs, ObjectiveDesc(DTO_OBJECTIVE_MINIMUM_TIME, Int32(0), Int32(0), Int32(0), w, o.D, null, null,
                                        Ptr{Int64}(C_NULL), 0, Ptr{Int32}(C_NULL), Int32(0), Int32(0), null, null,
                                        Ptr{Int32}(C_NULL), Int32(0), Int32(0)))
        elseif o isa GlobalObjective || o isa GlobalKnotPointObjective
            # closures over [z_t[var_names]; global_data[global_names]] (global_objectives.jl:35-350): blocks per listing, the
            # engine ACCUMULATES them (:270-271, :341); a GlobalObjective is one listing of the global variables alone
            comps1 = o isa GlobalKnotPointObjective ? vcat([collect(traj.components[n]) for n in o.var_names]...) : Int[]
            gcomps1 = vcat([collect(traj.global_components[n]) for n in o.global_names]...)
            comps, gcomps = Int32.(comps1 .- 1), Int32.(gcomps1 .- 1)
            times = o isa GlobalKnotPointObjective ? Vector{Int64}(o.times) : Int64[]
            push!(keep, comps, gcomps, times)
            push!(odescs, ObjectiveDesc(DTO_OBJECTIVE_EXTERNAL_GLOBAL, Int32(0), Int32(0), Int32(0), w, 0.0, null, null,
                                        isempty(times) ? Ptr{Int64}(C_NULL) : pointer(times), length(times),
                                        isempty(comps) ? Ptr{Int32}(C_NULL) : pointer(comps), Int32(length(comps)), Int32(0), null, null,
                                        pointer(gcomps), Int32(length(gcomps)), Int32(0)))
            push!(ext_objectives, o)
            ext_comps[o] = comps1
            ext_gcomps[o] = gcomps1
        elseif hasproperty(o, :var_names) && hasproperty(o, :times)   # KnotPointObjective / TerminalObjective: host closure
            comps1 = vcat([collect(traj.components[n]) for n in o.var_names]...)
            comps = Int32.(comps1 .- 1)
            times = Vector{Int64}(o.times)
            push!(keep, comps, times)
            push!(odescs, ObjectiveDesc(DTO_OBJECTIVE_EXTERNAL_KNOT, Int32(0), Int32(0), Int32(0), w, 0.0, null, null,
                                        pointer(times), length(times), pointer(comps), Int32(length(comps)), Int32(0), null, null,
                                        Ptr{Int32}(C_NULL), Int32(0), Int32(0)))
            push!(ext_objectives, o)
            ext_comps[o] = comps1
        else
            error("DTOEngine: objective term $(typeof(o)) is not supported; keep Solvers.Evaluator for this problem")
        end
    end

    # nonlinear constraints: rows follow the dynamics (evaluator.jl:219-223); closures -> EXTERNAL with the pattern of the
    # Jacobian at the initial point (evaluator.jl:136)
    cdescs = ConstraintDesc[]
    ext_constraints = Tuple{AbstractNonlinearConstraint,Int}[]
    for con in prob.constraints
        con isa AbstractNonlinearConstraint || continue   # linear constraints go to MOI directly (solve.jl)
        if con isa NonlinearGlobalConstraint
            # g(global_data[global_names]) (global_constraint.jl:20-160): patterns from the Jacobian and the Hessian of sum(g)
            # at the initial point (evaluator.jl:136, :166)
            gcomps1 = vcat([collect(traj.global_components[n]) for n in con.global_names]...)
            gcomps = Int32.(gcomps1 .- 1)
            g0 = Vector{Float64}(traj.global_data[gcomps1])
            jac0 = vec(Matrix{Float64}(ForwardDiff.jacobian(con.g, g0)))
            hess0 = vec(Matrix{Float64}(ForwardDiff.hessian(x -> sum(con.g(x)), g0)))
            push!(keep, gcomps, jac0, hess0)
            push!(cdescs, ConstraintDesc(DTO_CONSTRAINT_EXTERNAL_GLOBAL, Int32(con.equality), Int32(length(gcomps)), Int32(con.dim),
                                         pointer(gcomps), 0.0, Ptr{Int64}(C_NULL), 0, pointer(jac0), pointer(hess0)))
            push!(ext_constraints, (con, row))
            ext_gcomps[con] = gcomps1
            row += con.dim
            continue
        end
        if con isa QuadraticFormKnotConstraint   # built into the engine: nothing to evaluate or upload per callback
            comps = Int32.(vcat([collect(traj.components[n]) for n in con.var_names]...) .- 1)
            times = Vector{Int64}(con.times)
            M = vec(con.M)   # column-major n_comps x n_comps, rides in hess0
            push!(keep, comps, times, M)
            push!(cdescs, ConstraintDesc(DTO_CONSTRAINT_QUADFORM_MINUS_C, Int32(con.equality), Int32(length(comps)), Int32(1),
                                         pointer(comps), con.c, pointer(times), length(times), null, pointer(M)))
            row += con.dim
            continue
        end
        con isa NonlinearKnotPointConstraint || error("DTOEngine: constraint $(typeof(con)) is not supported")
        comps1 = vcat([collect(traj.components[n]) for n in con.var_names]...)
        comps = Int32.(comps1 .- 1)
        times = Vector{Int64}(con.times)
        J0 = eval_jacobian(con, traj)
        jac0 = knot_blocks(J0, con, comps1, traj)
        push!(keep, comps, times, jac0)
        push!(cdescs, ConstraintDesc(DTO_CONSTRAINT_EXTERNAL, Int32(con.equality), Int32(length(comps)), Int32(con.g_dim),
                                     pointer(comps), 0.0, pointer(times), length(times), pointer(jac0), null))
        push!(ext_constraints, (con, row))
        ext_comps[con] = comps1
        row += con.dim
    end

    Z0 = vcat(traj.datavec, traj.global_data)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve keep idescs odescs cdescs Z0 begin
        desc = Ref(ProblemDesc(DTO_ABI_VERSION, Int32(device), Int64(traj.N), Int32(traj.dim), Int32(traj.global_dim),
                               first0(traj, traj.timestep), Int32(eval_hessian), Int32(length(idescs)), Int32(length(odescs)),
                               Int32(length(cdescs)), (block_generators ? DTO_FLAG_BLOCK_GENERATORS : Int32(0)) | (shared_generators ? DTO_FLAG_SHARED_GENERATORS : Int32(0)), pointer(idescs), pointer(odescs), pointer(cdescs),
                               pointer(Z0), Int64(k_lo), Int64(k_hi)))
        rc = @ccall lib.dto_create(desc::Ptr{ProblemDesc}, h::Ptr{Ptr{Cvoid}})::Cint
        rc == 0 || error(unsafe_string(@ccall lib.dto_last_error(C_NULL::Ptr{Cvoid})::Cstring))
    end
    handle = h[]
    n = Ref{Int64}(0)
    @ccall lib.dto_num_vars(handle::Ptr{Cvoid}, n::Ptr{Int64})::Cint
    n_vars = Int(n[])
    @ccall lib.dto_num_cons(handle::Ptr{Cvoid}, n::Ptr{Int64})::Cint
    n_cons = Int(n[])
    @ccall lib.dto_num_dynamics_cons(handle::Ptr{Cvoid}, n::Ptr{Int64})::Cint
    @assert Int(n[]) == n_dyn
    function structure(count_fn, fill_fn)
        cnt = Ref{Int64}(0)
        count_fn(cnt)
        rows = Vector{Int64}(undef, cnt[])
        cols = Vector{Int64}(undef, cnt[])
        fill_fn(cnt[], rows, cols) == 0 || error("DTOEngine: structure query failed")
        return collect(zip(Int.(rows), Int.(cols)))
    end
    jstruct = structure(c -> (@ccall lib.dto_jac_nnz(handle::Ptr{Cvoid}, c::Ptr{Int64})::Cint),
                        (c, r, k) -> (@ccall lib.dto_jacobian_structure(handle::Ptr{Cvoid}, 0::Int64, c::Int64, r::Ptr{Int64}, k::Ptr{Int64})::Cint))
    hstruct = structure(c -> (@ccall lib.dto_hess_nnz(handle::Ptr{Cvoid}, c::Ptr{Int64})::Cint),
                        (c, r, k) -> (@ccall lib.dto_hessian_structure(handle::Ptr{Cvoid}, 0::Int64, c::Int64, r::Ptr{Int64}, k::Ptr{Int64})::Cint))
    ev = GPUEvaluator(handle, traj, n_vars, n_cons, n_dyn, n_cons - n_dyn, eval_hessian, jstruct, hstruct,
                      ext_integrators, ext_constraints, ext_objectives, ext_comps, ext_gcomps, Vector{Float64}[])
    finalizer(e -> (@ccall lib.dto_destroy(e.handle::Ptr{Cvoid})::Cvoid), ev)
    return ev
end

# ---- host-evaluated terms: the reference's own functions produce the blocks -----------------------------------------

# _update_trajectory_cache! of the reference (evaluator.jl:474-482)
function update!(ev::GPUEvaluator, Z::AbstractVector{Float64})
    traj = ev.trajectory
    nd = traj.dim * traj.N
    traj.datavec .= @view Z[1:nd]
    traj.global_dim > 0 && (traj.global_data .= @view Z[nd+1:end])
    return traj
end

# dense per-listing blocks (g_dim x n_comps, column-major, listing after listing) of a knot constraint's sparse Jacobian
function knot_blocks(J::SparseMatrixCSC, con::NonlinearKnotPointConstraint, comps1::Vector{Int}, traj::NamedTrajectory)
    out = Vector{Float64}(undef, con.g_dim * length(comps1) * length(con.times))
    p = 0
    for (i, t) in enumerate(con.times)
        blk = Matrix(J[slice(i, con.g_dim), slice(t, comps1, traj.dim)])
        out[p+1:p+length(blk)] .= vec(blk)
        p += length(blk)
    end
    return out
end

# need: 0 values, 1 + first derivatives, 2 + second derivatives; -1: this callback does not read that family
function stage_external!(ev::GPUEvaluator, Z::AbstractVector{Float64}; con_need::Int = -1, obj_need::Int = -1, μ = nothing)
    n_ext = length(ev.ext_integrators) + length(ev.ext_constraints) + length(ev.ext_objectives)
    n_ext == 0 && return nothing
    traj = update!(ev, Z)
    z = traj.dim
    vals = fill(ExternalValues(C_NULL, C_NULL, C_NULL), n_ext)
    empty!(ev.staging)
    stage(v::Vector{Float64}) = (push!(ev.staging, v); pointer(v))
    slot = 0
    for (integ, row) in ev.ext_integrators
        slot += 1
        con_need < 0 && continue
        δ = zeros(integ.dim)
        evaluate!(δ, integ, traj)
        jac_p = Ptr{Float64}(C_NULL)
        hess_p = Ptr{Float64}(C_NULL)
        if con_need >= 1
            J = eval_jacobian(integ, traj)
            blocks = Vector{Float64}(undef, integ.x_dim * 2z * (traj.N - 1))
            for k = 1:traj.N-1
                blocks[(k-1)*integ.x_dim*2z+1:k*integ.x_dim*2z] .= vec(Matrix(J[slice(k, integ.x_dim), slice(k, 1:2z, z)]))
            end
            jac_p = stage(blocks)
        end
        if con_need >= 2
            H = eval_hessian_of_lagrangian(integ, traj, μ[row:row+integ.dim-1])
            blocks = zeros(4 * z * z * (traj.N - 1))
            for k = 1:traj.N-1
                # one 2z x 2z block per interval; the reference's matrix holds the SUM of neighbouring intervals on the
                # shared diagonal block, so take interval k's own part: evaluate the integrator's blocks one by one
                blocks[(k-1)*4z*z+1:k*4z*z] .= vec(interval_hessian(integ, traj, μ[row:row+integ.dim-1], k, H))
            end
            hess_p = stage(blocks)
        end
        vals[slot] = ExternalValues(stage(δ), jac_p, hess_p)
    end
    for (con, row) in ev.ext_constraints
        slot += 1
        con_need < 0 && continue
        if con isa NonlinearGlobalConstraint   # one listing: values g, Jacobian g_dim x n_comps, Hessian of mu' g (global_constraint.jl:102-134)
            gv = Vector{Float64}(traj.global_data[ev.ext_gcomps[con]])
            jac_p = con_need >= 1 ? stage(vec(Matrix{Float64}(ForwardDiff.jacobian(con.g, gv)))) : Ptr{Float64}(C_NULL)
            μc = con_need >= 2 ? Vector{Float64}(μ[row:row+con.dim-1]) : Float64[]
            hess_p = con_need >= 2 ? stage(vec(Matrix{Float64}(ForwardDiff.hessian(x -> μc' * con.g(x), gv)))) : Ptr{Float64}(C_NULL)
            vals[slot] = ExternalValues(stage(Vector{Float64}(con.g(gv))), jac_p, hess_p)
            continue
        end
        g = zeros(con.dim)
        evaluate!(g, con, traj)
        jac_p = Ptr{Float64}(C_NULL)
        hess_p = Ptr{Float64}(C_NULL)
        comps1 = ev.ext_comps[con]
        con_need >= 1 && (jac_p = stage(knot_blocks(eval_jacobian(con, traj), con, comps1, traj)))
        if con_need >= 2
            H = eval_hessian_of_lagrangian(con, traj, μ[row:row+con.dim-1])
            nc = length(comps1)
            blocks = Vector{Float64}(undef, nc * nc * length(con.times))
            for (i, t) in enumerate(con.times)
                r = slice(t, comps1, z)
                blocks[(i-1)*nc*nc+1:i*nc*nc] .= vec(Matrix(H[r, r]))
            end
            hess_p = stage(blocks)
        end
        vals[slot] = ExternalValues(stage(g), jac_p, hess_p)
    end
    for o in ev.ext_objectives
        slot += 1
        obj_need < 0 && continue
        if o isa GlobalObjective || o isa GlobalKnotPointObjective
            # blocks over xg = [z_t[comps]; global_data[gcomps]] per listing, differentiated as the reference does
            # (ForwardDiff on the closure, global_objectives.jl:76-79, :117, :258, :330)
            gv = Vector{Float64}(traj.global_data[ev.ext_gcomps[o]])
            listings = o isa GlobalObjective ? [(x -> o.Q * o.ℓ(x), gv)] :
                [(let i = i; x -> o.Qs[i] * o.ℓ(x, o.params[i]) end, vcat(vcat([traj[t][n] for n in o.var_names]...), gv))
                 for (i, t) in enumerate(o.times)]
            v = Float64[f(x) for (f, x) in listings]
            grad_p = obj_need >= 1 ? stage(vcat([ForwardDiff.gradient(f, x) for (f, x) in listings]...)) : Ptr{Float64}(C_NULL)
            hess_p = obj_need >= 2 ? stage(vcat([vec(ForwardDiff.hessian(f, x)) for (f, x) in listings]...)) : Ptr{Float64}(C_NULL)
            vals[slot] = ExternalValues(stage(v), grad_p, hess_p)
            continue
        end
        comps1 = ev.ext_comps[o]
        nc = length(comps1)
        nt = length(o.times)
        v = [o.Qs[i] * o.ℓ(vcat([traj[t][n] for n in o.var_names]...), o.params[i]) for (i, t) in enumerate(o.times)]
        grad_p = Ptr{Float64}(C_NULL)
        hess_p = Ptr{Float64}(C_NULL)
        if obj_need >= 1
            ∇ = zeros(ev.n_variables)
            gradient!(∇, o, traj)   # overwrites per listed time (knot_point_objectives.jl:198): the engine keeps the last listing
            grad_p = stage(vcat([∇[slice(t, comps1, z)] for t in o.times]...))
        end
        if obj_need >= 2
            H = get_full_hessian(o, traj)
            H = H + triu(H, 1)'     # the reference returns the upper triangle (knot_point_objectives.jl:242)
            blocks = Vector{Float64}(undef, nc * nc * nt)
            for (i, t) in enumerate(o.times)
                r = slice(t, comps1, z)
                blocks[(i-1)*nc*nc+1:i*nc*nc] .= vec(Matrix(H[r, r]))
            end
            hess_p = stage(blocks)
        end
        vals[slot] = ExternalValues(stage(Vector{Float64}(v)), grad_p, hess_p)
    end
    n32 = Int32(n_ext)
    GC.@preserve vals check(ev, @ccall lib.dto_set_external(ev.handle::Ptr{Cvoid}, n32::Int32, vals::Ptr{ExternalValues})::Cint)
    return nothing
end

# interval k's own 2z x 2z Hessian block of an integrator: H holds sums on the shared diagonal blocks, so the own part of
# the z_k diagonal is recovered by subtracting what interval k-1 put there.  Integrators whose blocks do not touch their
# z_{k+1} diagonal (all of the reference's) need no correction; a user integrator that does should provide this method.
function interval_hessian(integ, traj, μ, k, H)
    z = traj.dim
    return Matrix(H[slice(k, 1:2z, z), slice(k, 1:2z, z)])
end

# ---- MOI surface (evaluator.jl:291-456) -----------------------------------------------------------------------------
MOI.initialize(::GPUEvaluator, features) = nothing
MOI.features_available(ev::GPUEvaluator) = ev.eval_hessian ? [:Grad, :Jac, :Hess, :HessVec] : [:Grad, :Jac]
MOI.jacobian_structure(ev::GPUEvaluator) = ev.jacobian_structure
MOI.hessian_lagrangian_structure(ev::GPUEvaluator) = ev.hessian_structure

function MOI.eval_objective(ev::GPUEvaluator, Z::AbstractVector{Float64})
    stage_external!(ev, Z; obj_need = 0)
    f = Ref{Float64}(0.0)
    GC.@preserve Z check(ev, @ccall lib.dto_eval_objective(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, f::Ptr{Float64})::Cint)
    return f[]
end

function MOI.eval_objective_gradient(ev::GPUEvaluator, ∇::AbstractVector{Float64}, Z::AbstractVector{Float64})
    stage_external!(ev, Z; obj_need = 1)
    GC.@preserve ∇ Z check(ev, @ccall lib.dto_eval_gradient(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, ∇::Ptr{Float64})::Cint)
    return nothing
end

function MOI.eval_constraint(ev::GPUEvaluator, g::AbstractVector{Float64}, Z::AbstractVector{Float64})
    stage_external!(ev, Z; con_need = 0)
    GC.@preserve g Z check(ev, @ccall lib.dto_eval_constraint(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, g::Ptr{Float64})::Cint)
    return nothing
end

function MOI.eval_constraint_jacobian(ev::GPUEvaluator, ∂::AbstractVector{Float64}, Z::AbstractVector{Float64})
    stage_external!(ev, Z; con_need = 1)
    GC.@preserve ∂ Z check(ev, @ccall lib.dto_eval_jacobian(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, ∂::Ptr{Float64})::Cint)
    return nothing
end

function MOI.eval_hessian_lagrangian(ev::GPUEvaluator, H::AbstractVector{Float64}, Z::AbstractVector{Float64}, σ::Float64, μ::AbstractVector{Float64})
    stage_external!(ev, Z; con_need = 2, obj_need = σ != 0 ? 2 : -1, μ = μ)
    GC.@preserve H Z μ check(ev, @ccall lib.dto_eval_hessian(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, σ::Float64, μ::Ptr{Float64}, H::Ptr{Float64})::Cint)
    return nothing
end

# h = H(Z; σ, μ) v (:HessVec): the engine assembles H once per point on the device and multiplies from a compact copy; products
# at the same (Z, σ, μ) cost one launch -- closure-based terms stage their blocks anew on every call, which starts a new point
function MOI.eval_hessian_lagrangian_product(ev::GPUEvaluator, h::AbstractVector{Float64}, Z::AbstractVector{Float64}, v::AbstractVector{Float64},
                                             σ::Float64, μ::AbstractVector{Float64})
    stage_external!(ev, Z; con_need = 2, obj_need = σ != 0 ? 2 : -1, μ = μ)
    GC.@preserve h Z v μ check(ev, @ccall lib.dto_eval_hessian_product(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, σ::Float64, μ::Ptr{Float64},
                                                                         v::Ptr{Float64}, h::Ptr{Float64})::Cint)
    return nothing
end

# y = J(Z) w and y = J(Z)' w (evaluator.jl:406-456): matrix-free on the device, no Jacobian crosses the bus
function MOI.eval_constraint_jacobian_product(ev::GPUEvaluator, y::AbstractVector{Float64}, Z::AbstractVector{Float64}, w::AbstractVector{Float64})
    stage_external!(ev, Z; con_need = 1)
    GC.@preserve y Z w check(ev, @ccall lib.dto_eval_jacobian_product(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, w::Ptr{Float64}, y::Ptr{Float64})::Cint)
    return nothing
end

function MOI.eval_constraint_jacobian_transpose_product(ev::GPUEvaluator, y::AbstractVector{Float64}, Z::AbstractVector{Float64}, w::AbstractVector{Float64})
    stage_external!(ev, Z; con_need = 1)
    GC.@preserve y Z w check(ev, @ccall lib.dto_eval_jacobian_transpose_product(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, w::Ptr{Float64}, y::Ptr{Float64})::Cint)
    return nothing
end

# ---- open-loop rollout on the device (include/dto_engine.h, "Open-loop rollout") ---------------------------------------------------
# X_{k+1} = E_k(Z) X_k through every interval of integrator `integrator` (0-based position in `prob.integrators`), E_k the propagator
# whose negative eval_constraint_jacobian stores: the states the dynamics reach from X0 under the controls of the iterate Z, whatever
# states Z holds.  The reference's rollout callbacks (callback_rollout_fidelity_factory, callback_best_rollout_fidelity_factory:
# src/solvers/ipopt_solver/callbacks.jl:264-361) call `fid_fn(problem.trajectory, system)` every `freq` iterations; a `fid_fn` on the
# engine closes over the evaluator and scores the rolled-out final state with the caller's own fidelity, e.g. for a ket
#     fid_fn = (traj, sys) -> iso_fidelity(vec(rollout(ev, vec(traj); all_knots = false)), ψ̃_goal)
# and for a unitary X0 = the identity of the isomorphic state (n_cols = x_dim) gives the cumulative propagator.
# `X0`: x_dim x n_cols (a Vector is one column); `nothing` takes the integrator's state at knot 1 of Z.  Returns x_dim x n_cols x N
# (knot 1 is a copy of X0), or x_dim x n_cols with `all_knots = false`: bit for bit the last slice.
function rollout(ev::GPUEvaluator, Z::AbstractVector{Float64}; integrator::Integer = 0, X0::Union{Nothing,AbstractVecOrMat{Float64}} = nothing,
                 all_knots::Bool = true)
    stage_external!(ev, Z; con_need = 1)
    i0 = Int32(integrator)
    b = Ref{Int32}(0); reps = Ref{Int32}(0); active = Ref{Int32}(0)
    check(ev, @ccall lib.dto_integrator_blocks(ev.handle::Ptr{Cvoid}, i0::Int32, b::Ptr{Int32}, reps::Ptr{Int32}, active::Ptr{Int32})::Cint)
    x_dim = Int(b[]) * Int(reps[])
    X0m = X0 === nothing ? nothing : Matrix{Float64}(reshape(X0, size(X0, 1), :))
    nc = Int32(X0m === nothing ? 1 : size(X0m, 2))
    mode = all_knots ? DTO_ROLLOUT_ALL : DTO_ROLLOUT_FINAL
    X = all_knots ? fill(NaN, x_dim, Int(nc), ev.trajectory.N) : fill(NaN, x_dim, Int(nc))
    p0 = X0m === nothing ? Ptr{Float64}(C_NULL) : pointer(X0m)
    GC.@preserve X Z X0m check(ev, @ccall lib.dto_rollout(ev.handle::Ptr{Cvoid}, i0::Int32, Z::Ptr{Float64}, p0::Ptr{Float64}, nc::Int32, mode::Int32,
                                                          X::Ptr{Float64})::Cint)
    return X
end

# the same on device pointers: dX0 x_dim x n_cols (or C_NULL with n_cols = 1), dX x_dim x n_cols x N (or x_dim x n_cols); enqueued on `stream`
function rollout_dev!(ev::GPUEvaluator, dX::Ptr{Float64}, dZ::Ptr{Float64}, dX0::Ptr{Float64}, n_cols::Integer, stream::Ptr{Cvoid};
                      integrator::Integer = 0, all_knots::Bool = true, Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 1)
    i0 = Int32(integrator)
    nc = Int32(n_cols)
    mode = all_knots ? DTO_ROLLOUT_ALL : DTO_ROLLOUT_FINAL
    check(ev, @ccall lib.dto_rollout_dev(ev.handle::Ptr{Cvoid}, i0::Int32, dZ::Ptr{Float64}, dX0::Ptr{Float64}, nc::Int32, mode::Int32,
                                         dX::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- solves with the dynamics block (include/dto_engine.h, "Solves with the dynamics block") ----------------------------------------
# Forward, the linearised rollout Y_1 = B_1, Y_{k+1} = E_k(Z) Y_k + B_{k+1}; with `adjoint = true` the costate recursion Λ_N = B_N,
# Λ_k = E_k(Z)' Λ_{k+1} + B_k.  `B`: x_dim x n_cols x N (a Matrix is one column per knot).  Returns x_dim x n_cols x N, or with
# `all_knots = false` the x_dim x n_cols block at knot N (forward) or knot 1 (adjoint), bit for bit that slice.  A second solve at the
# same Z -- in either direction -- reuses the product tree of the first and runs its scan alone.
function dynamics_solve(ev::GPUEvaluator, Z::AbstractVector{Float64}, B::AbstractArray{Float64}; integrator::Integer = 0, adjoint::Bool = false,
                        all_knots::Bool = true)
    stage_external!(ev, Z; con_need = 1)
    i0 = Int32(integrator)
    N = ev.trajectory.N
    Bm = Array{Float64,3}(ndims(B) == 3 ? B : reshape(B, size(B, 1), 1, :))
    size(Bm, 3) == N || error("dynamics_solve: B holds $(size(Bm, 3)) knots, the trajectory has $N")
    x_dim = size(Bm, 1)
    nc = Int32(size(Bm, 2))
    dir = adjoint ? DTO_SOLVE_ADJOINT : DTO_SOLVE_FORWARD
    mode = all_knots ? DTO_ROLLOUT_ALL : DTO_ROLLOUT_FINAL
    Y = all_knots ? fill(NaN, x_dim, Int(nc), N) : fill(NaN, x_dim, Int(nc))
    GC.@preserve Y Z Bm check(ev, @ccall lib.dto_dynamics_solve(ev.handle::Ptr{Cvoid}, i0::Int32, Z::Ptr{Float64}, dir::Int32, Bm::Ptr{Float64}, nc::Int32,
                                                                mode::Int32, Y::Ptr{Float64})::Cint)
    return Y
end

# the same on device pointers: dB x_dim x n_cols x N, dY x_dim x n_cols x N (or x_dim x n_cols); enqueued on `stream`
function dynamics_solve_dev!(ev::GPUEvaluator, dY::Ptr{Float64}, dZ::Ptr{Float64}, dB::Ptr{Float64}, n_cols::Integer, stream::Ptr{Cvoid};
                             integrator::Integer = 0, adjoint::Bool = false, all_knots::Bool = true, Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 1)
    i0 = Int32(integrator)
    nc = Int32(n_cols)
    dir = adjoint ? DTO_SOLVE_ADJOINT : DTO_SOLVE_FORWARD
    mode = all_knots ? DTO_ROLLOUT_ALL : DTO_ROLLOUT_FINAL
    check(ev, @ccall lib.dto_dynamics_solve_dev(ev.handle::Ptr{Cvoid}, i0::Int32, dZ::Ptr{Float64}, dir::Int32, dB::Ptr{Float64}, nc::Int32,
                                                mode::Int32, dY::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- whole-dynamics solves (include/dto_engine.h, "Whole-dynamics solves") -----------------------------------------------------------
# The Jacobian block of ALL integrators' rows and ALL their state columns, with identity rows for knot 1: what a reduced-space method
# eliminates the states with.  `dynamics_layout` returns (n_states, n_levels, offset, level): D = the sum of the integrators' state
# dimensions and, per integrator of `prob.integrators` (`n_integrators` = their number), its 0-based offset on the D axis and its
# dependency level.  It needs no device.
function dynamics_layout(ev::GPUEvaluator, n_integrators::Integer)
    n = Int(n_integrators)
    ns = Ref{Int32}(0); nl = Ref{Int32}(0)
    offset = zeros(Int32, max(n, 1)); level = zeros(Int32, max(n, 1))
    GC.@preserve offset level check(ev, @ccall lib.dto_dynamics_layout(ev.handle::Ptr{Cvoid}, ns::Ptr{Int32}, nl::Ptr{Int32}, offset::Ptr{Int32},
                                                                       level::Ptr{Int32})::Cint)
    return Int(ns[]), Int(nl[]), offset[1:n], level[1:n]
end

# Forward, the linearised rollout of the whole trajectory under fixed controls (B = -defect with zero knot-1 columns: the Newton state
# correction); with `adjoint = true` the costates of all dynamics rows, slice 1 the derivative with respect to the initial states.
# `B`: n_states x n_cols x N (a Matrix is one column per knot).  Returns n_states x n_cols x N.  A second solve at the same Z -- in
# either direction -- launches no Jacobian, gather or tree kernel.
function dynamics_solve_all(ev::GPUEvaluator, Z::AbstractVector{Float64}, B::AbstractArray{Float64}; adjoint::Bool = false)
    stage_external!(ev, Z; con_need = 1)
    N = ev.trajectory.N
    Bm = Array{Float64,3}(ndims(B) == 3 ? B : reshape(B, size(B, 1), 1, :))
    size(Bm, 3) == N || error("dynamics_solve_all: B holds $(size(Bm, 3)) knots, the trajectory has $N")
    nc = Int32(size(Bm, 2))
    dir = adjoint ? DTO_SOLVE_ADJOINT : DTO_SOLVE_FORWARD
    Y = fill(NaN, size(Bm, 1), Int(nc), N)
    GC.@preserve Y Z Bm check(ev, @ccall lib.dto_dynamics_solve_all(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, dir::Int32, Bm::Ptr{Float64}, nc::Int32,
                                                                    Y::Ptr{Float64})::Cint)
    return Y
end

# the same on device pointers: dB and dY n_states x n_cols x N, not overlapping; enqueued on `stream`
function dynamics_solve_all_dev!(ev::GPUEvaluator, dY::Ptr{Float64}, dZ::Ptr{Float64}, dB::Ptr{Float64}, n_cols::Integer, stream::Ptr{Cvoid};
                                 adjoint::Bool = false, Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 1)
    nc = Int32(n_cols)
    dir = adjoint ? DTO_SOLVE_ADJOINT : DTO_SOLVE_FORWARD
    check(ev, @ccall lib.dto_dynamics_solve_all_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, dir::Int32, dB::Ptr{Float64}, nc::Int32,
                                                    dY::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- reduced-space operators (include/dto_engine.h, "Reduced-space operators") ---------------------------------------------------------
# The gradient and the Hessian-vector product of the problem with the states eliminated by the dynamics: the control-only view of a
# GRAPE-style or truncated-Newton method.  `μ`: multipliers of all constraint rows (its dynamics rows are never read) or `nothing` for
# zeros.  The reduced point -- costates, multipliers, gradient -- is kept per (Z, σ, μ): products at the point of the last call run no
# Jacobian chain, tree build or Hessian assembly.
# Returns the reduced gradient (n_variables: zero on the states of knots 2 .. N, the costates of knot 1 on the states of knot 1), with
# `costates = true` also the costates as n_states x N, n_states asked of the handle (`dto_dynamics_layout`).
function reduced_check_lengths(ev::GPUEvaluator, who::String, Z, μ, v = nothing)
    length(Z) == ev.n_variables || error("$who: Z has $(length(Z)) entries, the problem has $(ev.n_variables) variables")
    μ === nothing || length(μ) == ev.n_constraints || error("$who: μ has $(length(μ)) entries, the problem has $(ev.n_constraints) constraints")
    v === nothing || length(v) == ev.n_variables || error("$who: v has $(length(v)) entries, the problem has $(ev.n_variables) variables")
    return nothing
end

function reduced_gradient(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,AbstractVector{Float64}} = nothing,
                          costates::Bool = false)
    reduced_check_lengths(ev, "reduced_gradient", Z, μ)
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    grad = fill(NaN, ev.n_variables)
    lam = zeros(Float64, 0, 0)
    if costates   # the costates' first dimension is the handle's own D (every array of dto_dynamics_layout may be NULL)
        ns = Ref{Int32}(0)
        check(ev, @ccall lib.dto_dynamics_layout(ev.handle::Ptr{Cvoid}, ns::Ptr{Int32}, C_NULL::Ptr{Int32}, C_NULL::Ptr{Int32},
                                                 C_NULL::Ptr{Int32})::Cint)
        lam = fill(NaN, Int(ns[]), ev.trajectory.N)
    end
    GC.@preserve grad lam Zv μv begin
        μp = μ === nothing ? Ptr{Float64}(C_NULL) : pointer(μv)
        lp = costates ? pointer(lam) : Ptr{Float64}(C_NULL)
        check(ev, @ccall lib.dto_reduced_gradient(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64},
                                                  grad::Ptr{Float64}, lp::Ptr{Float64})::Cint)
    end
    return costates ? (grad, lam) : grad
end

# y = T' H(Z; σ, μ~) T v: `v` and the result have n_variables entries; the entries of `v` at the states of knots 2 .. N are not read,
# those of the result are zero.
function reduced_hessian_product(ev::GPUEvaluator, Z::AbstractVector{Float64}, v::AbstractVector{Float64}; σ::Float64 = 1.0,
                                 μ::Union{Nothing,AbstractVector{Float64}} = nothing)
    reduced_check_lengths(ev, "reduced_hessian_product", Z, μ, v)
    Zv, vv = Vector{Float64}(Z), Vector{Float64}(v)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    y = fill(NaN, ev.n_variables)
    GC.@preserve y Zv vv μv begin
        μp = μ === nothing ? Ptr{Float64}(C_NULL) : pointer(μv)
        check(ev, @ccall lib.dto_reduced_hessian_product(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64},
                                                         vv::Ptr{Float64}, y::Ptr{Float64})::Cint)
    end
    return y
end

# the same on device pointers, enqueued on `stream`; dμ and dlam may be C_NULL
function reduced_gradient_dev!(ev::GPUEvaluator, dgrad::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dlam::Ptr{Float64},
                               stream::Ptr{Cvoid})
    check(ev, @ccall lib.dto_reduced_gradient_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dgrad::Ptr{Float64},
                                                  dlam::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function reduced_hessian_product_dev!(ev::GPUEvaluator, dy::Ptr{Float64}, dZ::Ptr{Float64}, dv::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64},
                                      stream::Ptr{Cvoid})
    check(ev, @ccall lib.dto_reduced_hessian_product_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dv::Ptr{Float64},
                                                         dy::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- block products (include/dto_engine.h, "Block products"): many vectors per call ---------------------------------------------------
# `V` is n_variables x n_cols (a column per vector: the engine's [n_cols][n_variables]); the result has the same shape, sized from the
# handle.  Column c is, bit for bit, the single product of column c; the engine reads the Hessian copy, the solves' node matrices and
# the input blocks once per chunk of columns (`set_option!(ev, "reduced_block_width", w)` caps the chunk, 0 = the engine's choice).
function block_check_lengths(ev::GPUEvaluator, who::String, Z, μ, V)
    reduced_check_lengths(ev, who, Z, μ)
    size(V, 1) == ev.n_variables || error("$who: V has $(size(V, 1)) rows, the problem has $(ev.n_variables) variables")
    size(V, 2) >= 1 || error("$who: V has no column")
    return nothing
end

# Y[:, c] = H(Z; σ, μ) V[:, c]
function eval_hessian_lagrangian_products(ev::GPUEvaluator, Z::AbstractVector{Float64}, V::AbstractMatrix{Float64}, σ::Float64,
                                          μ::AbstractVector{Float64})
    block_check_lengths(ev, "eval_hessian_lagrangian_products", Z, μ, V)
    stage_external!(ev, Z; con_need = 2, obj_need = σ != 0 ? 2 : -1, μ = μ)
    Zv, Vm, μv = Vector{Float64}(Z), Matrix{Float64}(V), Vector{Float64}(μ)
    Y = fill(NaN, ev.n_variables, size(Vm, 2))
    nc = Int32(size(Vm, 2))
    GC.@preserve Y Zv Vm μv check(ev, @ccall lib.dto_eval_hessian_products(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μv::Ptr{Float64},
                                                                          nc::Int32, Vm::Ptr{Float64}, Y::Ptr{Float64})::Cint)
    return Y
end

# Y[:, c] = T' H(Z; σ, μ~) T V[:, c]: the rows of `V` at the states of knots 2 .. N are not read, those of the result are zero
function reduced_hessian_products(ev::GPUEvaluator, Z::AbstractVector{Float64}, V::AbstractMatrix{Float64}; σ::Float64 = 1.0,
                                  μ::Union{Nothing,AbstractVector{Float64}} = nothing)
    block_check_lengths(ev, "reduced_hessian_products", Z, μ, V)
    Zv, Vm = Vector{Float64}(Z), Matrix{Float64}(V)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    Y = fill(NaN, ev.n_variables, size(Vm, 2))
    nc = Int32(size(Vm, 2))
    GC.@preserve Y Zv Vm μv begin
        μp = μ === nothing ? Ptr{Float64}(C_NULL) : pointer(μv)
        check(ev, @ccall lib.dto_projected_hessian_products(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, nc::Int32,
                                                            Vm::Ptr{Float64}, Y::Ptr{Float64})::Cint)
    end
    return Y
end

# the same on device pointers ([n_cols][n_variables] each, not overlapping), enqueued on `stream`; dμ of the projected form may be C_NULL
function eval_hessian_products_dev!(ev::GPUEvaluator, dY::Ptr{Float64}, dZ::Ptr{Float64}, dV::Ptr{Float64}, n_cols::Integer, σ::Float64,
                                    dμ::Ptr{Float64}, stream::Ptr{Cvoid})
    nc = Int32(n_cols)
    check(ev, @ccall lib.dto_eval_hessian_products_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, nc::Int32,
                                                       dV::Ptr{Float64}, dY::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function reduced_hessian_products_dev!(ev::GPUEvaluator, dY::Ptr{Float64}, dZ::Ptr{Float64}, dV::Ptr{Float64}, n_cols::Integer, σ::Float64,
                                       dμ::Ptr{Float64}, stream::Ptr{Cvoid})
    nc = Int32(n_cols)
    check(ev, @ccall lib.dto_projected_hessian_products_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, nc::Int32,
                                                            dV::Ptr{Float64}, dY::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- feasible trajectory and merit value (include/dto_engine.h, "Feasible trajectory") ------------------------------------------------
# Zf = Z with every integrator's states of knots 2 .. N replaced by what its dynamics reach from the states of knot 1: one engine call,
# one Jacobian evaluation per dependency level that holds a propagator.
function feasible_trajectory(ev::GPUEvaluator, Z::AbstractVector{Float64})
    reduced_check_lengths(ev, "feasible_trajectory", Z, nothing)
    stage_external!(ev, Z; con_need = 1)
    Zv = Vector{Float64}(Z)
    Zf = fill(NaN, ev.n_variables)
    GC.@preserve Zv Zf check(ev, @ccall lib.dto_feasible_trajectory(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, Zf::Ptr{Float64})::Cint)
    return Zf
end

# φ = σ f(Zf) + Σ over the non-dynamics rows of μ_r g_r(Zf), the function `reduced_gradient` and `reduced_hessian_product` are
# derivatives of; returns (φ, Zf, g) -- g holds every row at Zf, the dynamics rows being the defects the rollout leaves.
function feasible_merit(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,AbstractVector{Float64}} = nothing)
    reduced_check_lengths(ev, "feasible_merit", Z, μ)
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    φ = Ref{Float64}(NaN)
    Zf = fill(NaN, ev.n_variables)
    g = fill(NaN, ev.n_constraints)
    GC.@preserve Zv μv Zf g begin
        μp = μ === nothing ? Ptr{Float64}(C_NULL) : pointer(μv)
        check(ev, @ccall lib.dto_feasible_merit(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, φ::Ptr{Float64},
                                                Zf::Ptr{Float64}, g::Ptr{Float64})::Cint)
    end
    return φ[], Zf, g
end

# the same on device pointers, enqueued on `stream`; dZf may equal dZ (in place); dμ, and for the merit dZf and dg, may be C_NULL
function feasible_trajectory_dev!(ev::GPUEvaluator, dZf::Ptr{Float64}, dZ::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 1)
    check(ev, @ccall lib.dto_feasible_trajectory_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, dZf::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function feasible_merit_dev!(ev::GPUEvaluator, dφ::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dZf::Ptr{Float64},
                             dg::Ptr{Float64}, stream::Ptr{Cvoid})
    check(ev, @ccall lib.dto_feasible_merit_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dφ::Ptr{Float64},
                                                dZf::Ptr{Float64}, dg::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- truncated-Newton step (include/dto_engine.h, "Truncated-Newton step") ------------------------------------------------------------
# Steihaug-Toint CG on (M T'HT M + shift M) p = -M g in one engine call: g and T'HT the reduced gradient and Hessian at (Z, σ, μ), M
# zeroing the states of knots 2 .. N and the entries whose `free` value is 0.0.  Returns (p, info, trace): info the eight doubles of the
# header (status, iterations, ‖g‖, ‖r‖, ‖p‖, p⋅g, predicted decrease, last curvature), trace 4 x iterations (κ, d⋅d, s, r⋅r per column).
function newton_step(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,AbstractVector{Float64}} = nothing,
                     free::Union{Nothing,AbstractVector{Float64}} = nothing, radius::Float64 = 0.0, shift::Float64 = 0.0,
                     rtol::Float64 = 1e-6, atol::Float64 = 0.0, max_iter::Integer = 50)
    reduced_check_lengths(ev, "newton_step", Z, μ, free)
    max_iter >= 1 || error("newton_step: max_iter = $max_iter, at least 1 iteration is required")
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    fv = free === nothing ? Float64[] : Vector{Float64}(free)
    p = fill(NaN, ev.n_variables)
    info = fill(NaN, 8)
    trace = fill(NaN, 4, Int(max_iter))
    mi = Int32(max_iter)
    GC.@preserve Zv μv fv p info trace begin
        μp = μ === nothing ? Ptr{Float64}(C_NULL) : pointer(μv)
        fp = free === nothing ? Ptr{Float64}(C_NULL) : pointer(fv)
        check(ev, @ccall lib.dto_projected_newton_step(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, fp::Ptr{Float64},
                                                       radius::Float64, shift::Float64, rtol::Float64, atol::Float64, mi::Int32,
                                                       p::Ptr{Float64}, info::Ptr{Float64}, trace::Ptr{Float64})::Cint)
    end
    return p, info, trace[:, 1:Int(info[2])]
end

# the same on device pointers, on `stream` (one 16-byte readback per iteration); dμ, dfree and dtrace may be C_NULL
function newton_step_dev!(ev::GPUEvaluator, dp::Ptr{Float64}, dinfo::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64},
                          dfree::Ptr{Float64}, radius::Float64, shift::Float64, rtol::Float64, atol::Float64, max_iter::Integer,
                          dtrace::Ptr{Float64}, stream::Ptr{Cvoid})
    mi = Int32(max_iter)
    check(ev, @ccall lib.dto_projected_newton_step_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dfree::Ptr{Float64},
                                                           radius::Float64, shift::Float64, rtol::Float64, atol::Float64, mi::Int32,
                                                           dp::Ptr{Float64}, dinfo::Ptr{Float64}, dtrace::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- bound-constrained truncated-Newton step (include/dto_engine.h, "Bound-constrained truncated-Newton step") --------------------------
# newton_step with simple bounds lo <= Z + p <= hi on the independent entries (`lo`, `hi`: n_variables each or `nothing`; the data of
# the reference's BoundsConstraint expanded over the knots).  Returns (p, info, trace, states, Zp): info the twelve doubles of the header,
# trace 6 x iterations (κ, d⋅d, s, r⋅r over the free set, τ_box, entries hit), states the DTO_BOX_* codes as doubles (usable as the next
# call's `free`), Zp = Z + p with the entries that hit a bound holding it exactly.
const DTO_BOX_FIXED = Int32(0)
const DTO_BOX_FREE = Int32(1)
const DTO_BOX_HELD_LOWER = Int32(2)
const DTO_BOX_HELD_UPPER = Int32(3)
const DTO_BOX_HIT_LOWER = Int32(4)
const DTO_BOX_HIT_UPPER = Int32(5)

function newton_step_box(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,AbstractVector{Float64}} = nothing,
                         lo::Union{Nothing,AbstractVector{Float64}} = nothing, hi::Union{Nothing,AbstractVector{Float64}} = nothing,
                         free::Union{Nothing,AbstractVector{Float64}} = nothing, radius::Float64 = 0.0, shift::Float64 = 0.0,
                         rtol::Float64 = 1e-6, atol::Float64 = 0.0, max_iter::Integer = 50)
    reduced_check_lengths(ev, "newton_step_box", Z, μ, free)
    (lo === nothing || length(lo) == ev.n_variables) || error("newton_step_box: lo has $(length(lo)) entries, n_variables = $(ev.n_variables)")
    (hi === nothing || length(hi) == ev.n_variables) || error("newton_step_box: hi has $(length(hi)) entries, n_variables = $(ev.n_variables)")
    max_iter >= 1 || error("newton_step_box: max_iter = $max_iter, at least 1 iteration is required")
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    fv = free === nothing ? Float64[] : Vector{Float64}(free)
    lov = lo === nothing ? Float64[] : Vector{Float64}(lo)
    hiv = hi === nothing ? Float64[] : Vector{Float64}(hi)
    p = fill(NaN, ev.n_variables)
    info = fill(NaN, 12)
    trace = fill(NaN, 6, Int(max_iter))
    states = fill(NaN, ev.n_variables)
    Zp = fill(NaN, ev.n_variables)
    mi = Int32(max_iter)
    GC.@preserve Zv μv fv lov hiv p info trace states Zp begin
        μp = μ === nothing ? Ptr{Float64}(C_NULL) : pointer(μv)
        fp = free === nothing ? Ptr{Float64}(C_NULL) : pointer(fv)
        lop = lo === nothing ? Ptr{Float64}(C_NULL) : pointer(lov)
        hip = hi === nothing ? Ptr{Float64}(C_NULL) : pointer(hiv)
        check(ev, @ccall lib.dto_projected_newton_step_box(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, fp::Ptr{Float64},
                                                           lop::Ptr{Float64}, hip::Ptr{Float64}, radius::Float64, shift::Float64,
                                                           rtol::Float64, atol::Float64, mi::Int32, p::Ptr{Float64}, info::Ptr{Float64},
                                                           trace::Ptr{Float64}, states::Ptr{Float64}, Zp::Ptr{Float64})::Cint)
    end
    return p, info, trace[:, 1:Int(info[2])], states, Zp
end

# the same on device pointers, on `stream` (one 16-byte readback per iteration); dμ, dfree, dlo, dhi, dtrace, dstates and dZp may be C_NULL
function newton_step_box_dev!(ev::GPUEvaluator, dp::Ptr{Float64}, dinfo::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64},
                              dfree::Ptr{Float64}, dlo::Ptr{Float64}, dhi::Ptr{Float64}, radius::Float64, shift::Float64, rtol::Float64,
                              atol::Float64, max_iter::Integer, dtrace::Ptr{Float64}, dstates::Ptr{Float64}, dZp::Ptr{Float64},
                              stream::Ptr{Cvoid})
    mi = Int32(max_iter)
    check(ev, @ccall lib.dto_projected_newton_step_box_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dfree::Ptr{Float64},
                                                               dlo::Ptr{Float64}, dhi::Ptr{Float64}, radius::Float64, shift::Float64,
                                                               rtol::Float64, atol::Float64, mi::Int32, dp::Ptr{Float64}, dinfo::Ptr{Float64},
                                                               dtrace::Ptr{Float64}, dstates::Ptr{Float64}, dZp::Ptr{Float64},
                                                               stream::Ptr{Cvoid})::Cint)
end

# ---- augmented-Lagrangian terms (include/dto_engine.h, "Augmented-Lagrangian terms") ----------------------------------------------------
# The reduced-space calls above with a penalty ρ_r on the non-dynamics rows (Powell-Hestenes-Rockafellar: inequality rows g_r ≤ 0 by the
# constraint's `equality = false`).  `μ`, `ρ`: n_constraints each or `nothing` (μ: zeros; ρ: no penalties, the call is then the one it
# extends).  `penalty_vector(ev, value)` expands a value per constraint over the rows.
function auglag_ptr(x::Union{Nothing,AbstractVector{Float64}}, xv::Vector{Float64})
    return x === nothing ? Ptr{Float64}(C_NULL) : pointer(xv)
end

function auglag_check_lengths(ev::GPUEvaluator, who::String, Z, μ, ρ)
    reduced_check_lengths(ev, who, Z, μ)
    ρ === nothing || length(ρ) == ev.n_constraints || error("$who: ρ has $(length(ρ)) entries, the problem has $(ev.n_constraints) constraints")
    return nothing
end

# ρ over the rows: 0 in the dynamics rows, which come first; on the rows of constraint i (`constraint_rows[i]` of them, the constraints
# in list order) `value`, a number, or `value[i]` of a vector with one entry per constraint
function penalty_vector(ev::GPUEvaluator, value, constraint_rows::AbstractVector{<:Integer})
    n_dyn = ev.n_constraints - sum(constraint_rows)
    ρ = zeros(Float64, ev.n_constraints)
    row = n_dyn
    for (i, n) in enumerate(constraint_rows)
        ρ[row+1:row+n] .= value isa Number ? Float64(value) : Float64(value[i])
        row += n
    end
    return ρ
end

# the row pass at Z: (μ_eff, weight, info); μ_eff is the first-order multiplier update, info the eight doubles of the header
function auglag_rows(ev::GPUEvaluator, Z::AbstractVector{Float64}; μ::Union{Nothing,AbstractVector{Float64}} = nothing,
                     ρ::Union{Nothing,AbstractVector{Float64}} = nothing)
    auglag_check_lengths(ev, "auglag_rows", Z, μ, ρ)
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    ρv = ρ === nothing ? Float64[] : Vector{Float64}(ρ)
    μ_eff, weight, info = fill(NaN, ev.n_constraints), fill(NaN, ev.n_constraints), fill(NaN, 8)
    GC.@preserve Zv μv ρv μ_eff weight info begin
        μp, ρp = auglag_ptr(μ, μv), auglag_ptr(ρ, ρv)
        check(ev, @ccall lib.dto_auglag_rows(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, μp::Ptr{Float64}, ρp::Ptr{Float64}, μ_eff::Ptr{Float64},
                                             weight::Ptr{Float64}, info::Ptr{Float64})::Cint)
    end
    return μ_eff, weight, info
end

# Φ = σ f(Zf) + Σ ψ_r(g_r(Zf)) at the feasible trajectory Zf of Z: (Φ, Zf, g, info)
function auglag_merit(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,AbstractVector{Float64}} = nothing,
                      ρ::Union{Nothing,AbstractVector{Float64}} = nothing)
    auglag_check_lengths(ev, "auglag_merit", Z, μ, ρ)
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    ρv = ρ === nothing ? Float64[] : Vector{Float64}(ρ)
    Φ = Ref{Float64}(NaN)
    Zf, g, info = fill(NaN, ev.n_variables), fill(NaN, ev.n_constraints), fill(NaN, 8)
    GC.@preserve Zv μv ρv Zf g info begin
        μp, ρp = auglag_ptr(μ, μv), auglag_ptr(ρ, ρv)
        check(ev, @ccall lib.dto_auglag_merit(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, ρp::Ptr{Float64},
                                              Φ::Ptr{Float64}, Zf::Ptr{Float64}, g::Ptr{Float64}, info::Ptr{Float64})::Cint)
    end
    return Φ[], Zf, g, info
end

# the reduced gradient of Φ: (grad, μ_eff)
function auglag_gradient(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,AbstractVector{Float64}} = nothing,
                         ρ::Union{Nothing,AbstractVector{Float64}} = nothing)
    auglag_check_lengths(ev, "auglag_gradient", Z, μ, ρ)
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    ρv = ρ === nothing ? Float64[] : Vector{Float64}(ρ)
    grad, μ_eff = fill(NaN, ev.n_variables), fill(NaN, ev.n_constraints)
    lam = Ptr{Float64}(C_NULL)
    GC.@preserve Zv μv ρv grad μ_eff begin
        μp, ρp = auglag_ptr(μ, μv), auglag_ptr(ρ, ρv)
        check(ev, @ccall lib.dto_auglag_gradient(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, ρp::Ptr{Float64},
                                                 grad::Ptr{Float64}, lam::Ptr{Float64}, μ_eff::Ptr{Float64})::Cint)
    end
    return grad, μ_eff
end

# Y[:, c] = T'(H(Z; σ, μ~_eff) + J_c' W J_c) T V[:, c]
function auglag_hessian_products(ev::GPUEvaluator, Z::AbstractVector{Float64}, V::AbstractMatrix{Float64}; σ::Float64 = 1.0,
                                 μ::Union{Nothing,AbstractVector{Float64}} = nothing, ρ::Union{Nothing,AbstractVector{Float64}} = nothing)
    block_check_lengths(ev, "auglag_hessian_products", Z, μ, V)
    auglag_check_lengths(ev, "auglag_hessian_products", Z, μ, ρ)
    Zv, Vm = Vector{Float64}(Z), Matrix{Float64}(V)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    ρv = ρ === nothing ? Float64[] : Vector{Float64}(ρ)
    Y = fill(NaN, ev.n_variables, size(Vm, 2))
    nc = Int32(size(Vm, 2))
    GC.@preserve Y Zv Vm μv ρv begin
        μp, ρp = auglag_ptr(μ, μv), auglag_ptr(ρ, ρv)
        check(ev, @ccall lib.dto_auglag_hessian_products(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, ρp::Ptr{Float64},
                                                         nc::Int32, Vm::Ptr{Float64}, Y::Ptr{Float64})::Cint)
    end
    return Y
end

function auglag_hessian_product(ev::GPUEvaluator, Z::AbstractVector{Float64}, v::AbstractVector{Float64}; σ::Float64 = 1.0,
                                μ::Union{Nothing,AbstractVector{Float64}} = nothing, ρ::Union{Nothing,AbstractVector{Float64}} = nothing)
    return vec(auglag_hessian_products(ev, Z, reshape(Vector{Float64}(v), :, 1); σ = σ, μ = μ, ρ = ρ))
end

# newton_step_box on the augmented Lagrangian: (p, info, trace, states, Zp) as there
function auglag_newton_step(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,AbstractVector{Float64}} = nothing,
                            ρ::Union{Nothing,AbstractVector{Float64}} = nothing, lo::Union{Nothing,AbstractVector{Float64}} = nothing,
                            hi::Union{Nothing,AbstractVector{Float64}} = nothing, free::Union{Nothing,AbstractVector{Float64}} = nothing,
                            radius::Float64 = 0.0, shift::Float64 = 0.0, rtol::Float64 = 1e-6, atol::Float64 = 0.0, max_iter::Integer = 50)
    reduced_check_lengths(ev, "auglag_newton_step", Z, μ, free)
    auglag_check_lengths(ev, "auglag_newton_step", Z, μ, ρ)
    (lo === nothing || length(lo) == ev.n_variables) || error("auglag_newton_step: lo has $(length(lo)) entries, n_variables = $(ev.n_variables)")
    (hi === nothing || length(hi) == ev.n_variables) || error("auglag_newton_step: hi has $(length(hi)) entries, n_variables = $(ev.n_variables)")
    max_iter >= 1 || error("auglag_newton_step: max_iter = $max_iter, at least 1 iteration is required")
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    ρv = ρ === nothing ? Float64[] : Vector{Float64}(ρ)
    fv = free === nothing ? Float64[] : Vector{Float64}(free)
    lov = lo === nothing ? Float64[] : Vector{Float64}(lo)
    hiv = hi === nothing ? Float64[] : Vector{Float64}(hi)
    p, info, trace = fill(NaN, ev.n_variables), fill(NaN, 12), fill(NaN, 6, Int(max_iter))
    states, Zp = fill(NaN, ev.n_variables), fill(NaN, ev.n_variables)
    mi = Int32(max_iter)
    GC.@preserve Zv μv ρv fv lov hiv p info trace states Zp begin
        μp, ρp, fp, lop, hip = auglag_ptr(μ, μv), auglag_ptr(ρ, ρv), auglag_ptr(free, fv), auglag_ptr(lo, lov), auglag_ptr(hi, hiv)
        check(ev, @ccall lib.dto_auglag_newton_step(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, ρp::Ptr{Float64},
                                                    fp::Ptr{Float64}, lop::Ptr{Float64}, hip::Ptr{Float64}, radius::Float64, shift::Float64,
                                                    rtol::Float64, atol::Float64, mi::Int32, p::Ptr{Float64}, info::Ptr{Float64},
                                                    trace::Ptr{Float64}, states::Ptr{Float64}, Zp::Ptr{Float64})::Cint)
    end
    return p, info, trace[:, 1:Int(info[2])], states, Zp
end

# the same on device pointers, enqueued on `stream`; every pointer but dZ (and the required outputs) may be C_NULL
function auglag_rows_dev!(ev::GPUEvaluator, dμ_eff::Ptr{Float64}, dweight::Ptr{Float64}, dinfo::Ptr{Float64}, dZ::Ptr{Float64}, dμ::Ptr{Float64},
                          dρ::Ptr{Float64}, stream::Ptr{Cvoid})
    check(ev, @ccall lib.dto_auglag_rows_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, dμ::Ptr{Float64}, dρ::Ptr{Float64}, dμ_eff::Ptr{Float64},
                                             dweight::Ptr{Float64}, dinfo::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function auglag_merit_dev!(ev::GPUEvaluator, dΦ::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64}, dZf::Ptr{Float64},
                           dg::Ptr{Float64}, dinfo::Ptr{Float64}, stream::Ptr{Cvoid})
    check(ev, @ccall lib.dto_auglag_merit_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                                              dΦ::Ptr{Float64}, dZf::Ptr{Float64}, dg::Ptr{Float64}, dinfo::Ptr{Float64},
                                              stream::Ptr{Cvoid})::Cint)
end

function auglag_gradient_dev!(ev::GPUEvaluator, dgrad::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                              dlam::Ptr{Float64}, dμ_eff::Ptr{Float64}, stream::Ptr{Cvoid})
    check(ev, @ccall lib.dto_auglag_gradient_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                                                 dgrad::Ptr{Float64}, dlam::Ptr{Float64}, dμ_eff::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function auglag_hessian_products_dev!(ev::GPUEvaluator, dY::Ptr{Float64}, dZ::Ptr{Float64}, dV::Ptr{Float64}, n_cols::Integer, σ::Float64,
                                      dμ::Ptr{Float64}, dρ::Ptr{Float64}, stream::Ptr{Cvoid})
    nc = Int32(n_cols)
    check(ev, @ccall lib.dto_auglag_hessian_products_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                                                         nc::Int32, dV::Ptr{Float64}, dY::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function auglag_newton_step_dev!(ev::GPUEvaluator, dp::Ptr{Float64}, dinfo::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64},
                                 dρ::Ptr{Float64}, dfree::Ptr{Float64}, dlo::Ptr{Float64}, dhi::Ptr{Float64}, radius::Float64, shift::Float64,
                                 rtol::Float64, atol::Float64, max_iter::Integer, dtrace::Ptr{Float64}, dstates::Ptr{Float64}, dZp::Ptr{Float64},
                                 stream::Ptr{Cvoid})
    mi = Int32(max_iter)
    check(ev, @ccall lib.dto_auglag_newton_step_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                                                    dfree::Ptr{Float64}, dlo::Ptr{Float64}, dhi::Ptr{Float64}, radius::Float64,
                                                    shift::Float64, rtol::Float64, atol::Float64, mi::Int32, dp::Ptr{Float64},
                                                    dinfo::Ptr{Float64}, dtrace::Ptr{Float64}, dstates::Ptr{Float64}, dZp::Ptr{Float64},
                                                    stream::Ptr{Cvoid})::Cint)
end

# ---- L-BFGS preconditioner of the truncated-Newton step (include/dto_engine.h, "Preconditioned truncated-Newton step") ---------
# set_option!(ev, "newton_pairs", m), m = 0 .. 16 (0, the default: off), sets the capacity of the pair store and clears it.
function newton_pairs_push!(ev::GPUEvaluator, s::AbstractVector{Float64}, y::AbstractVector{Float64})
    (length(s) == ev.n_variables && length(y) == ev.n_variables) ||
        error("newton_pairs_push!: s and y have $(length(s)) and $(length(y)) entries, n_variables = $(ev.n_variables)")
    sv, yv = Vector{Float64}(s), Vector{Float64}(y)
    check(ev, @ccall lib.dto_newton_pairs_push(ev.handle::Ptr{Cvoid}, sv::Ptr{Float64}, yv::Ptr{Float64})::Cint)
end

function newton_pairs_push_dev!(ev::GPUEvaluator, ds::Ptr{Float64}, dy::Ptr{Float64}, stream::Ptr{Cvoid})
    check(ev, @ccall lib.dto_newton_pairs_push_dev(ev.handle::Ptr{Cvoid}, ds::Ptr{Float64}, dy::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

newton_pairs_clear!(ev::GPUEvaluator) = check(ev, @ccall lib.dto_newton_pairs_clear(ev.handle::Ptr{Cvoid})::Cint)

# (count, capacity)
function newton_pairs_info(ev::GPUEvaluator)
    count, cap = Ref{Int32}(0), Ref{Int32}(0)
    check(ev, @ccall lib.dto_newton_pairs_info(ev.handle::Ptr{Cvoid}, count::Ptr{Int32}, cap::Ptr{Int32})::Cint)
    return Int(count[]), Int(cap[])
end

# z = P H P r for the columns of R (n_variables x n_cols) with the store's pairs; free: the optional mask
function newton_precondition(ev::GPUEvaluator, R::AbstractMatrix{Float64}; free::Union{Nothing,AbstractVector{Float64}} = nothing)
    size(R, 1) == ev.n_variables || error("newton_precondition: R has $(size(R, 1)) rows, n_variables = $(ev.n_variables)")
    (free === nothing || length(free) == ev.n_variables) || error("newton_precondition: free has $(length(free)) entries, n_variables = $(ev.n_variables)")
    Rm = Matrix{Float64}(R)
    fv = free === nothing ? Float64[] : Vector{Float64}(free)
    Zm = fill(NaN, size(Rm))
    nc = Int32(size(Rm, 2))
    GC.@preserve Rm fv Zm begin
        fp = auglag_ptr(free, fv)
        check(ev, @ccall lib.dto_newton_precondition(ev.handle::Ptr{Cvoid}, fp::Ptr{Float64}, nc::Int32, Rm::Ptr{Float64}, Zm::Ptr{Float64})::Cint)
    end
    return Zm
end
newton_precondition(ev::GPUEvaluator, r::AbstractVector{Float64}; free = nothing) =
    vec(newton_precondition(ev, reshape(Vector{Float64}(r), :, 1); free = free))

function newton_precondition_dev!(ev::GPUEvaluator, dz::Ptr{Float64}, dr::Ptr{Float64}, n_cols::Integer, dfree::Ptr{Float64}, stream::Ptr{Cvoid})
    nc = Int32(n_cols)
    check(ev, @ccall lib.dto_newton_precondition_dev(ev.handle::Ptr{Cvoid}, dfree::Ptr{Float64}, nc::Int32, dr::Ptr{Float64}, dz::Ptr{Float64},
                                                     stream::Ptr{Cvoid})::Cint)
end

# auglag_newton_step (ρ = nothing: newton_step_box) preconditioned with the store's pairs: (p, info [16], trace [8 x iterations], states,
# Zp); harvest = true keeps this call's CG pairs as the next call's store
function preconditioned_newton_step(ev::GPUEvaluator, Z::AbstractVector{Float64}; σ::Float64 = 1.0,
                                    μ::Union{Nothing,AbstractVector{Float64}} = nothing, ρ::Union{Nothing,AbstractVector{Float64}} = nothing,
                                    lo::Union{Nothing,AbstractVector{Float64}} = nothing, hi::Union{Nothing,AbstractVector{Float64}} = nothing,
                                    free::Union{Nothing,AbstractVector{Float64}} = nothing, radius::Float64 = 0.0, shift::Float64 = 0.0,
                                    rtol::Float64 = 1e-6, atol::Float64 = 0.0, max_iter::Integer = 50, harvest::Bool = false)
    reduced_check_lengths(ev, "preconditioned_newton_step", Z, μ, free)
    auglag_check_lengths(ev, "preconditioned_newton_step", Z, μ, ρ)
    (lo === nothing || length(lo) == ev.n_variables) || error("preconditioned_newton_step: lo has $(length(lo)) entries, n_variables = $(ev.n_variables)")
    (hi === nothing || length(hi) == ev.n_variables) || error("preconditioned_newton_step: hi has $(length(hi)) entries, n_variables = $(ev.n_variables)")
    max_iter >= 1 || error("preconditioned_newton_step: max_iter = $max_iter, at least 1 iteration is required")
    Zv = Vector{Float64}(Z)
    μv = μ === nothing ? Float64[] : Vector{Float64}(μ)
    ρv = ρ === nothing ? Float64[] : Vector{Float64}(ρ)
    fv = free === nothing ? Float64[] : Vector{Float64}(free)
    lov = lo === nothing ? Float64[] : Vector{Float64}(lo)
    hiv = hi === nothing ? Float64[] : Vector{Float64}(hi)
    p, info, trace = fill(NaN, ev.n_variables), fill(NaN, 16), fill(NaN, 8, Int(max_iter))
    states, Zp = fill(NaN, ev.n_variables), fill(NaN, ev.n_variables)
    mi, hv = Int32(max_iter), Int32(harvest)
    GC.@preserve Zv μv ρv fv lov hiv p info trace states Zp begin
        μp, ρp, fp, lop, hip = auglag_ptr(μ, μv), auglag_ptr(ρ, ρv), auglag_ptr(free, fv), auglag_ptr(lo, lov), auglag_ptr(hi, hiv)
        check(ev, @ccall lib.dto_preconditioned_newton_step(ev.handle::Ptr{Cvoid}, Zv::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, ρp::Ptr{Float64},
                                                            fp::Ptr{Float64}, lop::Ptr{Float64}, hip::Ptr{Float64}, radius::Float64,
                                                            shift::Float64, rtol::Float64, atol::Float64, mi::Int32, hv::Int32,
                                                            p::Ptr{Float64}, info::Ptr{Float64}, trace::Ptr{Float64}, states::Ptr{Float64},
                                                            Zp::Ptr{Float64})::Cint)
    end
    return p, info, trace[:, 1:Int(info[2])], states, Zp
end

function preconditioned_newton_step_dev!(ev::GPUEvaluator, dp::Ptr{Float64}, dinfo::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64},
                                         dρ::Ptr{Float64}, dfree::Ptr{Float64}, dlo::Ptr{Float64}, dhi::Ptr{Float64}, radius::Float64,
                                         shift::Float64, rtol::Float64, atol::Float64, max_iter::Integer, harvest::Bool, dtrace::Ptr{Float64},
                                         dstates::Ptr{Float64}, dZp::Ptr{Float64}, stream::Ptr{Cvoid})
    mi, hv = Int32(max_iter), Int32(harvest)
    check(ev, @ccall lib.dto_preconditioned_newton_step_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                                                            dfree::Ptr{Float64}, dlo::Ptr{Float64}, dhi::Ptr{Float64}, radius::Float64,
                                                            shift::Float64, rtol::Float64, atol::Float64, mi::Int32, hv::Int32,
                                                            dp::Ptr{Float64}, dinfo::Ptr{Float64}, dtrace::Ptr{Float64}, dstates::Ptr{Float64},
                                                            dZp::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# ---- reduced-space minimize (include/dto_engine.h, "Reduced-space minimize") ------------------------------------------------
const DTO_MINIMIZE_CONVERGED = Int32(0)    # reduced_minimize!: status in info[1]
const DTO_MINIMIZE_MAX_OUTER = Int32(1)
const DTO_MINIMIZE_MAX_TRIALS = Int32(2)
const DTO_MINIMIZE_RADIUS = Int32(3)
const DTO_MINIMIZE_NOT_FINITE = Int32(4)
const DTO_MIN_OPTIONS = Int32(16)
# the options in index order (DTO_MIN_OPT_*, 0-based in the header) and their defaults
const MINIMIZE_OPTION_NAMES = (:radius0, :eta_accept, :eta_shrink, :eta_grow, :shrink_div, :grow_mul, :radius_max, :radius_min, :gtol, :ctol,
                               :viol_div, :rho_mul, :shift, :rtol, :atol, :max_iter)
const MINIMIZE_OPTION_DEFAULTS = (1.0, 0.1, 0.25, 0.75, 4.0, 2.0, Inf, 0.0, 0.0, 0.0, 4.0, 10.0, 0.0, 1e-6, 0.0, 50.0)

function minimize_options(options)
    for k in keys(options)
        k in MINIMIZE_OPTION_NAMES || error("reduced_minimize!: unknown option $k; the options are $(MINIMIZE_OPTION_NAMES)")
    end
    return Float64[Float64(get(options, k, d)) for (k, d) in zip(MINIMIZE_OPTION_NAMES, MINIMIZE_OPTION_DEFAULTS)]
end

# The trust-region loop around the step and the merit -- with ρ the outer multiplier / penalty loop around it -- as one device-resident
# call.  Z (and with ρ: μ, ρ) are updated IN PLACE; returns (info [16], history [8 x trials run], outer_history [4 x outer], states).
function reduced_minimize!(ev::GPUEvaluator, Z::Vector{Float64}; σ::Float64 = 1.0, μ::Union{Nothing,Vector{Float64}} = nothing,
                           ρ::Union{Nothing,Vector{Float64}} = nothing, lo::Union{Nothing,AbstractVector{Float64}} = nothing,
                           hi::Union{Nothing,AbstractVector{Float64}} = nothing, free::Union{Nothing,AbstractVector{Float64}} = nothing,
                           outer::Integer = 1, trials::Integer = 10, harvest::Bool = false, options...)
    reduced_check_lengths(ev, "reduced_minimize!", Z, μ, free)
    auglag_check_lengths(ev, "reduced_minimize!", Z, μ, ρ)
    (lo === nothing || length(lo) == ev.n_variables) || error("reduced_minimize!: lo has $(length(lo)) entries, n_variables = $(ev.n_variables)")
    (hi === nothing || length(hi) == ev.n_variables) || error("reduced_minimize!: hi has $(length(hi)) entries, n_variables = $(ev.n_variables)")
    (outer >= 1 && trials >= 1) || error("reduced_minimize!: outer = $outer, trials = $trials, at least 1 of each is required")
    opts = minimize_options(options)
    μv = μ === nothing ? Float64[] : μ
    ρv = ρ === nothing ? Float64[] : ρ
    fv = free === nothing ? Float64[] : Vector{Float64}(free)
    lov = lo === nothing ? Float64[] : Vector{Float64}(lo)
    hiv = hi === nothing ? Float64[] : Vector{Float64}(hi)
    info, history, outer_history = fill(NaN, 16), fill(NaN, 8, Int(outer) * Int(trials)), fill(NaN, 4, Int(outer))
    states = fill(NaN, ev.n_variables)
    no, nt, hv = Int32(outer), Int32(trials), Int32(harvest)
    GC.@preserve Z μv ρv fv lov hiv opts info history outer_history states begin
        μp, ρp, fp, lop, hip = auglag_ptr(μ, μv), auglag_ptr(ρ, ρv), auglag_ptr(free, fv), auglag_ptr(lo, lov), auglag_ptr(hi, hiv)
        check(ev, @ccall lib.dto_projected_minimize(ev.handle::Ptr{Cvoid}, Z::Ptr{Float64}, σ::Float64, μp::Ptr{Float64}, ρp::Ptr{Float64},
                                                  fp::Ptr{Float64}, lop::Ptr{Float64}, hip::Ptr{Float64}, opts::Ptr{Float64}, no::Int32,
                                                  nt::Int32, hv::Int32, info::Ptr{Float64}, history::Ptr{Float64},
                                                  outer_history::Ptr{Float64}, states::Ptr{Float64})::Cint)
    end
    passes = ρ === nothing ? 0 : Int(info[2]) - (Int(info[1]) == DTO_MINIMIZE_NOT_FINITE ? 1 : 0)
    return info, history[:, 1:Int(info[3])], outer_history[:, 1:passes], states
end

# device pointers, updated in place on `stream`; opts: the sixteen options on the HOST (as minimize_options builds them)
function reduced_minimize_dev!(ev::GPUEvaluator, dZ::Ptr{Float64}, dinfo::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                               dfree::Ptr{Float64}, dlo::Ptr{Float64}, dhi::Ptr{Float64}, opts::Vector{Float64}, outer::Integer, trials::Integer,
                               harvest::Bool, dhistory::Ptr{Float64}, douter_history::Ptr{Float64}, dstates::Ptr{Float64}, stream::Ptr{Cvoid})
    length(opts) == 16 || error("reduced_minimize_dev!: opts has $(length(opts)) entries, 16 are required (minimize_options)")
    no, nt, hv = Int32(outer), Int32(trials), Int32(harvest)
    GC.@preserve opts begin
        check(ev, @ccall lib.dto_projected_minimize_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dρ::Ptr{Float64},
                                                      dfree::Ptr{Float64}, dlo::Ptr{Float64}, dhi::Ptr{Float64}, opts::Ptr{Float64}, no::Int32,
                                                      nt::Int32, hv::Int32, dinfo::Ptr{Float64}, dhistory::Ptr{Float64},
                                                      douter_history::Ptr{Float64}, dstates::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
    end
end

# row bounds handed to the solver (src/solvers/solve.jl:30-65)
function constraint_bounds(ev::GPUEvaluator)
    lo = Vector{Float64}(undef, ev.n_constraints)
    hi = Vector{Float64}(undef, ev.n_constraints)
    check(ev, @ccall lib.dto_constraint_bounds(ev.handle::Ptr{Cvoid}, lo::Ptr{Float64}, hi::Ptr{Float64})::Cint)
    return lo, hi
end

# ---- device-resident entry points (MadNLP GPU mode, src/solvers/madnlp_solver/options.jl:12-16) ---------------------------
# Pointers are DEVICE pointers (e.g. `Ptr{Float64}(UInt(pointer(A)))` of an AMDGPU.ROCArray{Float64}), `stream` the HIP
# stream of those arrays; outputs stay in HBM and the call returns with its last kernels in flight on `stream`.  Closure-based
# terms are evaluated on the host: pass the host copy of Z (and of mu) as `Z_host` / `μ_host` for problems that have any.
function eval_objective_dev!(ev::GPUEvaluator, df::Ptr{Float64}, dZ::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; obj_need = 0)
    check(ev, @ccall lib.dto_eval_objective_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, df::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end
function eval_objective_gradient_dev!(ev::GPUEvaluator, d∇::Ptr{Float64}, dZ::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; obj_need = 1)
    check(ev, @ccall lib.dto_eval_gradient_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, d∇::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end
function eval_constraint_dev!(ev::GPUEvaluator, dg::Ptr{Float64}, dZ::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 0)
    check(ev, @ccall lib.dto_eval_constraint_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, dg::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end
function eval_constraint_jacobian_dev!(ev::GPUEvaluator, d∂::Ptr{Float64}, dZ::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 1)
    check(ev, @ccall lib.dto_eval_jacobian_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, d∂::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end
function eval_hessian_lagrangian_dev!(ev::GPUEvaluator, dH::Ptr{Float64}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, stream::Ptr{Cvoid};
                                      Z_host = nothing, μ_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 2, obj_need = σ != 0 ? 2 : -1, μ = μ_host)
    check(ev, @ccall lib.dto_eval_hessian_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dH::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function eval_hessian_lagrangian_product_dev!(ev::GPUEvaluator, dh::Ptr{Float64}, dZ::Ptr{Float64}, dv::Ptr{Float64}, σ::Float64,
                                              dμ::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing, μ_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 2, obj_need = σ != 0 ? 2 : -1, μ = μ_host)
    check(ev, @ccall lib.dto_eval_hessian_product_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, σ::Float64, dμ::Ptr{Float64}, dv::Ptr{Float64},
                                                      dh::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

# y = J(Z) w and y = J(Z)' w on device pointers (dw / dy: n_variables / n_constraints doubles, swapped for the transpose)
function eval_constraint_jacobian_product_dev!(ev::GPUEvaluator, dy::Ptr{Float64}, dZ::Ptr{Float64}, dw::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 1)
    check(ev, @ccall lib.dto_eval_jacobian_product_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, dw::Ptr{Float64}, dy::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

function eval_constraint_jacobian_transpose_product_dev!(ev::GPUEvaluator, dy::Ptr{Float64}, dZ::Ptr{Float64}, dw::Ptr{Float64}, stream::Ptr{Cvoid}; Z_host = nothing)
    Z_host === nothing || stage_external!(ev, Z_host; con_need = 1)
    check(ev, @ccall lib.dto_eval_jacobian_transpose_product_dev(ev.handle::Ptr{Cvoid}, dZ::Ptr{Float64}, dw::Ptr{Float64}, dy::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
end

"Declare a device value vector (DTO_VECTOR_JACOBIAN / DTO_VECTOR_HESSIAN) that the `*_dev!` calls are handed every iteration: its call-invariant entries are then written once (include/dto_engine.h, bound outputs).  `C_NULL` unbinds."
bind_output_dev!(ev::GPUEvaluator, vector::Int32, dptr::Ptr{Float64}) =
    check(ev, @ccall lib.dto_bind_output_dev(ev.handle::Ptr{Cvoid}, vector::Int32, dptr::Ptr{Float64})::Cint)

# ---- multi-GPU: one Julia process per GPU, `k_lo` / `k_hi` at construction; the engine owns the RCCL communicator --------------
# (SURVEY.md section 8e; BASELINE configs[3]).  No callback needs a collective; these gather the per-rank value slabs for a
# consumer that wants the whole vector on every GPU, and sum the objective's per-shard partial sums.
"128 bytes from ncclGetUniqueId: call on ONE rank, hand them to the others (MPI.bcast, a file, a socket)."
function comm_unique_id()
    id = zeros(UInt8, DTO_COMM_ID_BYTES)
    rc = @ccall lib.dto_comm_unique_id(id::Ptr{Cvoid})::Cint
    rc == 0 || error(unsafe_string(@ccall lib.dto_last_error(C_NULL::Ptr{Cvoid})::Cstring))
    return id
end
"Collective over the ranks: ncclCommInitRank on this handle's device + exchange of the ranks' knot ranges (rank is 0-based)."
function comm_create!(ev::GPUEvaluator, id::Vector{UInt8}, rank::Integer, world::Integer)
    r32, w32 = Int32(rank), Int32(world)
    GC.@preserve id check(ev, @ccall lib.dto_comm_create(ev.handle::Ptr{Cvoid}, id::Ptr{Cvoid}, r32::Int32, w32::Int32)::Cint)
end
comm_destroy!(ev::GPUEvaluator) = check(ev, @ccall lib.dto_comm_destroy(ev.handle::Ptr{Cvoid})::Cint)
"How to allocate one value vector (DTO_VECTOR_*) so that ONE in-place ncclAllGather moves every rank's slab: `padded_len` doubles; the vector starts at `front_pad`, this rank's slab at `front_pad + own_lo` (0-based offsets)."
function gather_layout(ev::GPUEvaluator, vector::Int32)
    L = Ref(GatherLayout(0, 0, 0, 0, 0, Int32(0), Int32(0)))
    check(ev, @ccall lib.dto_get_gather_layout(ev.handle::Ptr{Cvoid}, vector::Int32, L::Ptr{GatherLayout})::Cint)
    return L[]
end
gather_jacobian_dev!(ev::GPUEvaluator, dbuf::Ptr{Float64}, stream::Ptr{Cvoid}) =
    check(ev, @ccall lib.dto_gather_jacobian_dev(ev.handle::Ptr{Cvoid}, dbuf::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
gather_hessian_dev!(ev::GPUEvaluator, dbuf::Ptr{Float64}, stream::Ptr{Cvoid}) =
    check(ev, @ccall lib.dto_gather_hessian_dev(ev.handle::Ptr{Cvoid}, dbuf::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
gather_gradient_dev!(ev::GPUEvaluator, dbuf::Ptr{Float64}, stream::Ptr{Cvoid}) =
    check(ev, @ccall lib.dto_gather_gradient_dev(ev.handle::Ptr{Cvoid}, dbuf::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
gather_constraint_dev!(ev::GPUEvaluator, dg_local::Ptr{Float64}, dg_full::Ptr{Float64}, stream::Ptr{Cvoid}) =
    check(ev, @ccall lib.dto_gather_constraint_dev(ev.handle::Ptr{Cvoid}, dg_local::Ptr{Float64}, dg_full::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)
allreduce_objective_dev!(ev::GPUEvaluator, df::Ptr{Float64}, stream::Ptr{Cvoid}) =
    check(ev, @ccall lib.dto_allreduce_objective_dev(ev.handle::Ptr{Cvoid}, df::Ptr{Float64}, stream::Ptr{Cvoid})::Cint)

"""
`(block_dim, reps, active)` of integrator `i` (1-based): the finest replicated-block structure `G_j = I_reps ⊗ B_j` the engine found
in the generators it extracted from the closure (`GPUEvaluator(prob; block_generators = true)`: the `I(levels) ⊗ G̃(a)` of a unitary
in isomorphic coordinates; for a device `TimeDependentBilinearIntegrator` the structure shared by every `G_j` and carrier matrix `H_cj`)
and whether the structured path serves it; `(x_dim, 1, false)` otherwise.
"""
function integrator_blocks(ev::GPUEvaluator, i::Integer)
    b, r, a = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    i0 = Int32(i - 1)
    check(ev, @ccall lib.dto_integrator_blocks(ev.handle::Ptr{Cvoid}, i0::Int32, b::Ptr{Int32}, r::Ptr{Int32}, a::Ptr{Int32})::Cint)
    return Int(b[]), Int(r[]), a[] != 0
end

"""
`(leader, group_size, active)` of integrator `i` (1-based): the group of `BilinearIntegrator`s whose extracted generators and control
component are equal (`GPUEvaluator(prob; shared_generators = true)`: the kets `ψ̃1 … ψ̃P` of a multi-state problem, all built from
one closure `G`), its first member in list order, and whether the group shares one propagator chain in
`eval_constraint_jacobian`; `(i, 1, false)` otherwise.  The flag also groups device `TimeDependentBilinearIntegrator`s among
themselves -- the same generator family (every `G_j`, `H_cj`, modulation kind and frequency), control and time component, spline
order and sub-steps: at 65..256 states on the dense path such a group runs one propagation per `eval_constraint`, Jacobian and
Hessian call instead of one per ket (`set_option!(ev, "tdb_share_members", 1)` is one launch per member), with values bit-identical
to the unflagged evaluator's.
"""
function integrator_share(ev::GPUEvaluator, i::Integer)
    l, n, a = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    i0 = Int32(i - 1)
    check(ev, @ccall lib.dto_integrator_share(ev.handle::Ptr{Cvoid}, i0::Int32, l::Ptr{Int32}, n::Ptr{Int32}, a::Ptr{Int32})::Cint)
    return Int(l[]) + 1, Int(n[]), a[] != 0
end

"""
Flop model of one `eval_constraint_jacobian` per interval (`dto_interval_costs`): squarings of the propagator chain and Taylor
terms of the sweep from the growth bound of every `Δt_k G(u_k)` (the work of the reference's `expv`, bilinear_integrator.jl:81,
grows with that norm as well).  `balanced_knot_ranges` turns it into contiguous knot ranges of equal cost for `world` ranks --
SURVEY.md section 8e: on a pulse whose amplitude varies along the trajectory equal knot counts leave the slowest rank setting the
step.  Ranges of unequal length are gathered in the broadcast form (`gather_layout` then reports `in_place_all_gather == 0`).
"""
function interval_costs(ev::GPUEvaluator, Z⃗::AbstractVector{Float64})
    K = ev.trajectory.N - 1
    cost = Vector{Float64}(undef, K)
    Zc = convert(Vector{Float64}, Z⃗)
    first0, cnt = Int64(0), Int64(K)
    GC.@preserve Zc cost check(ev, @ccall lib.dto_interval_costs(ev.handle::Ptr{Cvoid}, Zc::Ptr{Float64}, first0::Int64, cnt::Int64, cost::Ptr{Float64})::Cint)
    return cost
end
function balanced_knot_ranges(cost::AbstractVector{Float64}, world::Integer)
    N = length(cost) + 1
    c = vcat(cost, 0.0)                      # the last knot owns no interval
    pre = vcat(0.0, cumsum(c))
    function parts(limit)
        cuts = Tuple{Int,Int}[]; lo = 0
        for r in 1:world
            left = world - r
            hi = searchsortedlast(pre, pre[lo + 1] + limit) - 1
            hi = max(lo + 1, min(hi, N - left))
            r == world && (hi = N)
            push!(cuts, (lo + 1, hi)); lo = hi
        end
        return cuts, maximum(pre[b + 1] - pre[a] for (a, b) in cuts)
    end
    lo_l, hi_l = max(maximum(c), pre[end] / world), pre[end]
    best = parts(hi_l)
    for _ in 1:60
        mid = (lo_l + hi_l) / 2
        cand = parts(mid)
        if cand[2] <= mid * (1 + 1e-12)
            best, hi_l = cand, mid
        else
            lo_l = mid
        end
    end
    return best[1]                            # [(k_lo, k_hi)] 1-based inclusive, one per rank
end

# dto_set_option (include/dto_engine.h lists the names), e.g. set_option!(ev, "tdb_matrix_free_products", 1): J w / J' w of device
# TimeDependentBilinearIntegrators (dense or structured path) without a value slab; set_option!(ev, "reduced_input_store", 1):
# reduced_gradient / reduced_hessian_product take J v^ and J' w from the input blocks kept with the whole-dynamics solves' point
# set_option!(ev, "reduced_block_width", 8): at most 8 columns per chunk of the block products (0 = the engine's choice)
function set_option!(ev::GPUEvaluator, name::AbstractString, value::Integer)
    v64 = Int64(value)
    check(ev, @ccall lib.dto_set_option(ev.handle::Ptr{Cvoid}, name::Cstring, v64::Int64)::Cint)
end

end # module

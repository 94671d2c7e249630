# HankHIP.jl — the reference-side binding a maintainer of vasudeva-ram/Julia-NewtonRaphsonHANK would add:
# the SAME Julia signatures as BackwardIteration.jl / ForwardIteration.jl, bodies replaced by `ccall`s
# into libhank_hip.so (include/hank_hip.h). `include` it AFTER the reference's own files; NewtonRaphson.jl,
# ModelParser.jl, SteadyState.jl and the YAML stay untouched.
#
# NOT EXERCISED IN THIS REPOSITORY'S CI: no Julia toolchain exists in the build image (SURVEY.md §8c).
# The C ABI it binds is exercised through the Python ctypes binding (julia-newtonraphsonhank_amd/hip.py),
# which makes exactly the same calls.
#
#   policy_seqs = BackwardIteration(x, exog_paths, mod, ss_end)          # BackwardIteration.jl:46-49
#   agg_seqs    = ForwardIteration(policy_seqs, mod, ss_initial)         # ForwardIteration.jl:253-255
#
# With x::Vector{Float64} both run the fused Float64 sweep (hank_primal); with
# x::Vector{ForwardDiff.Dual{T,Float64,N}} the N partials travel as one tangent batch (hank_jvp), so
# `JVP(fullFunction, x, y)` (GeneralStructures.jl:542-550) and ForwardDiff.jacobian chunks work unchanged.

using ForwardDiff: Dual, Partials, value, partials, tagtype

const LIBHANK = get(ENV, "HANK_HIP_LIB", joinpath(@__DIR__, "..", "julia-newtonraphsonhank_amd", "libhank_hip.so"))

struct HankModelC            # mirrors `hank_model` in include/hank_hip.h
    n_a::Int32; n_e::Int32; T::Int32; value_fn_id::Int32
    a_grid::Ptr{Float64}; z_grid::Ptr{Float64}; Pi::Ptr{Float64}
    beta::Float64; gamma::Float64; borrow_cons::Float64
end

mutable struct HankCtx
    ptr::Ptr{Cvoid}
    P::Int; G::Int; n_a::Int; n_e::Int
    hh_rows::Tuple        # names of the xVals rows the native family reads, in the order the library expects
    outputs::Tuple        # the heterogeneous variables the family returns, in the order of hank_get_het_outputs
    n_groups::Int         # group outputs the context holds (hank_set_group_outputs): the readers size their arrays by it
end

# native kernel families by value-function name: id (include/hank_hip.h), the household inputs it reads, and the heterogeneous
# variables it returns (output 1 = the policy variable of the endogenous dimension, output 2 = consumption, the c_grid of
# KrusellSmith.jl:79 returned as a second policy, output 3 = Value = (1+r) c^-γ, KrusellSmith.jl:80, output 4 = UCE = z_e c^-γ:
# hank_get_het_outputs)
const _FAMILIES = Dict(:ValueFunction => (0, (:r, :w), (:KD, :C, :Value)),                  # KrusellSmith.jl:43-83, :53-54
                       :HANKValueFunction => (1, (:r, :om, :Tr), (:A, :C, :Value, :UCE)))  # one-asset HANK (not in the reference)

# declare how many of the family's outputs the next hank_get_het_outputs reads (BackwardIteration.jl:99-112 keeps one sequence per
# key listed under `heterogeneous:`); the outputs up to the last listed key
_n_het(ctx::HankCtx, het_keys) = maximum(k -> findfirst(==(Symbol(k)), ctx.outputs), het_keys)
hank_set_het_outputs(ctx::HankCtx, n_het::Integer) =
    _check(ctx.ptr, ccall((:hank_set_het_outputs, LIBHANK), Cint, (Ptr{Cvoid}, Int32), ctx.ptr, Int32(n_het)))

# one device context per (SequenceModel, HIP device); device -1 = the current one. Keyed on the model ITSELF (an IdDict keeps it
# alive: an objectid can be recycled by a later model and hand it a context built for other grids) and guarded by a lock:
# sharded_jvp_columns reaches it from several tasks.
const _CTX = IdDict{Any,Dict{Int,HankCtx}}()
const _CTX_LOCK = ReentrantLock()

function _check(ctx::Ptr{Cvoid}, rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:hank_last_error, LIBHANK), Cstring, (Ptr{Cvoid},), ctx))
    error(msg)      # the library's messages restate the reference's own exceptions (knots / DomainError)
end

# `device`: HIP device ordinal (hank_create_on) — one context per GPU of a node lets ONE Julia process shard the columns of
# a tangent batch over the GPUs (sharded_jvp_columns below); `nothing` = the calling thread's current device (hank_create)
function hank_context(model::SequenceModel; device::Union{Nothing,Integer} = nothing)
    lock(_CTX_LOCK) do
    get!(get!(() -> Dict{Int,HankCtx}(), _CTX, model), device === nothing ? -1 : Int(device)) do
        w = model.heterogeneity.wealth; p = model.heterogeneity.productivity
        a = collect(Float64, w.grid); z = collect(Float64, p.grid); Π = Matrix{Float64}(p.transition)
        haskey(_FAMILIES, nameof(model.value_fn)) || error("no native kernel family for $(model.value_fn)")
        fam_id, rows, outs = _FAMILIES[nameof(model.value_fn)]
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve a z Π begin
            m = HankModelC(w.n, p.n, model.compspec.T, fam_id, pointer(a), pointer(z), pointer(Π),
                           model.params.β, model.params.γ, model.params.borrow_cons)
            rc = device === nothing ?
                ccall((:hank_create, LIBHANK), Cint, (Ref{HankModelC}, Ref{Ptr{Cvoid}}), m, ref) :
                ccall((:hank_create_on, LIBHANK), Cint, (Ref{HankModelC}, Int32, Ref{Ptr{Cvoid}}), m, Int32(device), ref)
        end
        _check(ref[], rc)
        ctx = HankCtx(ref[], model.compspec.T - 1, w.n * p.n, w.n, p.n, rows, outs, 0)
        @assert ccall((:hank_n_hh, LIBHANK), Cint, (Ptr{Cvoid},), ref[]) == length(rows)
        finalizer(c -> ccall((:hank_destroy, LIBHANK), Cint, (Ptr{Cvoid},), c.ptr), ctx)
        ctx
    end
    end
end

# rows of xVals the value function reads (KS: r_t, w_t, KrusellSmith.jl:53-54)
function _household_inputs(xVec_endog, model)
    @unpack T, n_endog = model.compspec
    xMat = reshape(xVec_endog, n_endog, T - 1)
    ek = vars_of_type(model, :endogenous)
    rows = [findfirst(==(k), ek) for k in hank_context(model).hh_rows]
    return xMat[rows, :]                                      # n_hh x (T-1), eltype of x
end

# What BackwardIteration returns: the reference's NamedTuple-of-Vector{Matrix} surface (seqs.KD[t]),
# copied from HBM on demand. The reference calls BackwardIteration with FOUR positionals
# (NewtonRaphson.jl:78) — `ss_initial` only reaches ForwardIteration (:79) — and the fused device sweep
# needs D_0, so the device call is DEFERRED: ForwardIteration runs the one fused sweep; reading a policy
# matrix before that runs it with a placeholder D_0 (policies do not depend on D_0).
mutable struct DevicePolicySeqs{TF}
    ctx::HankCtx; het_keys::Tuple; N::Int
    xhh::Matrix{Float64}; dxhh::Union{Nothing,Array{Float64,3}}; value::Matrix{Float64}
    D0::Union{Nothing,Vector{Float64}}; agg::Union{Nothing,Vector{Float64}}; dagg::Union{Nothing,Matrix{Float64}}
    aggs::Union{Nothing,Matrix{Float64}}; daggs::Union{Nothing,Array{Float64,3}}      # (P, n_het), (P, n_het, N): models with two heterogeneous variables
    grids::Tuple{Vector{Float64},Vector{Float64}}                                      # wealth and productivity grids (consumption policy)
end

# a Dual of the caller's own type TF = Dual{Tag,Float64,N} from a value and N partials: the inner
# constructor takes a Partials (ForwardDiff.jl/src/dual.jl:14-21); Dual{Tag}(v, ::Partials) is the
# public form (:59-66). There is no TF(value, p1, ..., pN) method.
@inline _mkdual(::Type{TF}, v::Float64, p::NTuple{N,Float64}) where {N,TF<:Dual} = Dual{tagtype(TF)}(v, Partials(p))

function _run_block!(s::DevicePolicySeqs, D0::Vector{Float64})
    ctx = s.ctx
    _check(ctx.ptr, ccall((:hank_set_boundary, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, s.value, D0))
    length(s.het_keys) > 1 && hank_set_het_outputs(ctx, max(_n_het(ctx, s.het_keys), 2))
    agg = Vector{Float64}(undef, ctx.P)
    dagg = nothing
    if s.dxhh === nothing
        _check(ctx.ptr, ccall((:hank_primal, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, s.xhh, agg))
    else      # a Dual pass carries value and partials together (NewtonRaphson.jl:95): one dual-sweep call
        dagg = Matrix{Float64}(undef, ctx.P, s.N)
        _check(ctx.ptr, ccall((:hank_primal_jvp, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                              ctx.ptr, s.xhh, s.dxhh, s.N, agg, dagg))
    end
    s.D0, s.agg, s.dagg = D0, agg, dagg
    if length(s.het_keys) > 1     # every heterogeneous variable's aggregate, reduced by the same sweeps (ForwardIteration.jl:303-307)
        n_het = _n_het(ctx, s.het_keys)
        s.aggs = Matrix{Float64}(undef, ctx.P, n_het)
        s.daggs = s.dxhh === nothing ? nothing : Array{Float64}(undef, ctx.P, n_het, s.N)
        _check(ctx.ptr, ccall((:hank_get_het_outputs, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                              ctx.ptr, Int32(n_het), s.dxhh === nothing ? C_NULL : s.dxhh, Int32(s.N), s.aggs, s.daggs === nothing ? C_NULL : s.daggs))
    end
    return s
end

# same positional signature as BackwardIteration.jl:46-49. No device work happens here (see above);
# `ss_initial` (optional keyword, not in the reference) runs the fused sweep straight away.
function BackwardIteration(xVec_endog, exog_paths::NamedTuple, model::SequenceModel, ss_end; ss_initial = nothing)
    ctx = hank_context(model)
    TF = eltype(xVec_endog)
    xd = _household_inputs(xVec_endog, model)
    xhh = Matrix{Float64}(value.(xd))
    N = TF <: Dual ? length(partials(first(xVec_endog))) : 0
    dxhh = N > 0 ? Float64[partials(xd[k, t])[n] for k in 1:size(xd, 1), t in 1:ctx.P, n in 1:N] : nothing   # (n_hh, P, N)
    s = DevicePolicySeqs{TF}(ctx, vars_of_type(model, :heterogeneous), N, xhh, dxhh, Matrix{Float64}(ss_end.value),
                             nothing, nothing, nothing, nothing, nothing,
                             (collect(Float64, model.heterogeneity.wealth.grid), collect(Float64, model.heterogeneity.productivity.grid)))
    ss_initial === nothing || _run_block!(s, Vector{Float64}(ss_initial.D))
    return s
end

# seqs.KD -> Vector of T-1 (Dual) matrices, as in the reference (BackwardIteration.jl:110-115)
function Base.getproperty(s::DevicePolicySeqs{TF}, k::Symbol) where {TF}
    k in fieldnames(DevicePolicySeqs) && return getfield(s, k)
    ctx = getfield(s, :ctx); N = getfield(s, :N)
    getfield(s, :agg) === nothing && _run_block!(s, fill(1.0 / ctx.G, ctx.G))     # read before ForwardIteration
    pol = Array{Float64}(undef, ctx.n_a, ctx.n_e, ctx.P)
    _check(ctx.ptr, ccall((:hank_get_policy_seq, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, pol))
    seq = if N == 0
        [pol[:, :, t] for t in 1:ctx.P]
    else
        dpol = Array{Float64}(undef, ctx.n_a, ctx.n_e, ctx.P, N)
        _check(ctx.ptr, ccall((:hank_get_dpolicy_seq, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), ctx.ptr, N, dpol))
        [[_mkdual(TF, pol[a, e, t], ntuple(n -> dpol[a, e, t, n], N)) for a in 1:ctx.n_a, e in 1:ctx.n_e] for t in 1:ctx.P]
    end
    k == ctx.outputs[1] && return seq
    k == :C || error("the native family returns $(ctx.outputs), not :$k")
    # consumption, the budget residual of KrusellSmith.jl:79: (1 + r) .* policy_a .+ (w .* labor_mat [.+ tr]) .- griddedpolicy
    xhh = getfield(s, :xhh); dxhh = getfield(s, :dxhh)
    xin(j, t) = N == 0 ? xhh[j, t] : _mkdual(TF, xhh[j, t], ntuple(n -> dxhh[j, t, n], N))
    grid = getfield(s, :grids)[1]; z = getfield(s, :grids)[2]
    return [[(1 + xin(1, t)) * grid[a] + (xin(2, t) * z[e] + (size(xhh, 1) > 2 ? xin(3, t) : 0.0)) - seq[t][a, e]
             for a in 1:ctx.n_a, e in 1:ctx.n_e] for t in 1:ctx.P]
end

# same signature as ForwardIteration.jl:253-255 for sequences that came from BackwardIteration above:
# this is where the ONE fused sweep of a fullFunction evaluation runs (NewtonRaphson.jl:78-79)
function ForwardIteration(seqs::DevicePolicySeqs{TF}, model::SequenceModel, ss_initial) where {TF}
    all(k -> k in seqs.ctx.outputs, seqs.het_keys) || error("the native family returns $(seqs.ctx.outputs) (got $(seqs.het_keys))")
    D0 = Vector{Float64}(ss_initial.D)
    (seqs.agg === nothing || D0 != seqs.D0) && _run_block!(seqs, D0)
    if length(seqs.het_keys) == 1
        agg, dagg = seqs.agg, seqs.dagg
        out = seqs.N == 0 ? agg : [_mkdual(TF, agg[t], ntuple(n -> dagg[t, n], seqs.N)) for t in 1:length(agg)]
        return NamedTuple{seqs.het_keys}((out,))
    end
    # one aggregate per heterogeneous variable, each its own policy dotted with the same D_t (ForwardIteration.jl:303-307)
    aggs, daggs = seqs.aggs, seqs.daggs
    col(k) = findfirst(==(k), seqs.ctx.outputs)
    outs = map(seqs.het_keys) do k
        j = col(k)
        seqs.N == 0 ? aggs[:, j] : [_mkdual(TF, aggs[t, j], ntuple(n -> daggs[t, j, n], seqs.N)) for t in 1:size(aggs, 1)]
    end
    return NamedTuple{seqs.het_keys}(Tuple(outs))
end

# ---- one process, several GPUs (GeneralStructures.jl:542-550: JVP is linear in `tangent`, so tangent columns shard) ----------
# dagg = J_household(x) * dxhh, the (P, N) household-block part of N JVPs at once, columns split over `devices`. Every
# context replays the (cheap) Float64 sweep; GPU g takes the contiguous column block g; each task blocks in its own
# `hank_primal_jvp` while the other GPUs run; the blocks land in ONE host matrix — no collective. This is what replaces the
# column loop of `getSteadyStateJacobian` (SteadyStateJacobian.jl:240-243) or a `ForwardDiff.jacobian` chunk loop.
function sharded_jvp_columns(model::SequenceModel, ss_end, ss_initial, xhh::Matrix{Float64}, dxhh::Array{Float64,3}; devices = [0])
    P, N, W = size(dxhh, 2), size(dxhh, 3), length(devices)
    dagg = Matrix{Float64}(undef, P, N)
    base, extra = divrem(N, W)
    value = Matrix{Float64}(ss_end.value); D0 = Vector{Float64}(ss_initial.D)
    ctxs = [hank_context(model; device = dev) for dev in devices]      # resolved (or created) on the calling task, before any task is spawned
    # (the blocking ccalls only overlap when Julia runs at least length(devices) threads: `julia -t N`; with one thread the tasks
    # serialise — then drive the contexts through the asynchronous hank_*_dev entries instead)
    @sync for (g, dev) in enumerate(devices)
        lo = (g - 1) * base + min(g - 1, extra) + 1
        hi = lo + base + (g <= extra ? 1 : 0) - 1
        hi < lo && continue
        Threads.@spawn begin                     # a context is used by ONE task at a time; different contexts run concurrently
            ctx = ctxs[g]
            _check(ctx.ptr, ccall((:hank_set_boundary, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, value, D0))
            agg = Vector{Float64}(undef, P)
            blk = dxhh[:, :, lo:hi]
            out = Matrix{Float64}(undef, P, hi - lo + 1)
            _check(ctx.ptr, ccall((:hank_primal_jvp, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                                  ctx.ptr, xhh, blk, Int32(hi - lo + 1), agg, out))
            dagg[:, lo:hi] = out
        end
    end
    return dagg
end

# The same with the blocks left in HBM and assembled on ONE GPU over xGMI (hank_gather_columns): `d_blocks[k]` is the device pointer
# of context k's (P, N_k[k]) block as hank_jvp_dev / hank_primal_jvp_dev wrote it, `d_out` a (P, sum N_k) buffer on ctxs[1]'s device.
# Asynchronous: hank_sync(ctxs[1]) — or work on its stream — sees the assembled matrix.
function gather_columns!(ctxs::Vector{HankCtx}, d_blocks::Vector{Ptr{Float64}}, N_k::Vector{Int32}, d_out::Ptr{Float64})
    ptrs = Ptr{Cvoid}[c.ptr for c in ctxs]
    _check(ctxs[1].ptr, ccall((:hank_gather_columns, LIBHANK), Cint, (Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Float64}}, Ptr{Int32}, Ptr{Float64}),
                              ptrs, Int32(length(ctxs)), d_blocks, N_k, d_out))
    return d_out
end

# which kernel family ran the last tangent sweep and how the context is configured (hank_info): (last_tangent_family, wide_mode,
# wide_min, wide_supported, xjvp_max, record_diet, record_bytes, 0); families: 0 per-period launches, 1 XCD-persistent, 2 on-chip wide
function hank_info(ctx::HankCtx)
    out = zeros(Int64, 8)
    _check(ctx.ptr, ccall((:hank_info, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Int64}), ctx.ptr, out))
    return out
end

# ---- the household block of getSteadyStateJacobian (SteadyStateJacobian.jl:187-256, :293-323, :358-387) ------------------------
# JBI (n_endog forward-mode JVPs through BackwardIteration seeded at the last period, :240-243), JFI (Zygote pullbacks
# through ForwardIteration, :249-253) and helper = JFI * JBI (:300-305) collapse into ONE call: hank_fake_news returns the
# fake-news matrix F[u, j, k] and the direct term Dv[j, k] of the household block at the steady state; the Toeplitz
# recursion (:363-371) stays here. Returns J[t, s, k] = d agg_t / d xhh_{k,s} (xhh rows in the order of `ctx.hh_rows`);
# the caller places it behind the equations' direct blocks (:124-145) exactly where `helper` goes today.
# A model that lists more than one heterogeneous variable (or one that is not the policy variable) takes hank_fake_news_het:
# every output is dotted with the same D_t (ForwardIteration.jl:303-307), so one set of sweeps serves all of them; the result
# is then a Dict of such J per heterogeneous key (the reference's slicing, :295-303, assumes one variable).
function household_jacobian_toeplitz(model::SequenceModel, ss; device = nothing)
    ctx = hank_context(model; device = device)
    P = ctx.P; n_hh = length(ctx.hh_rows)
    xhh = Float64[ss.vars[k] for k in ctx.hh_rows, _ in 1:P]                      # the constant steady-state path (:53-57)
    _check(ctx.ptr, ccall((:hank_set_boundary, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr,
                          Matrix{Float64}(ss.value), Vector{Float64}(ss.D)))
    agg = Vector{Float64}(undef, P)
    _check(ctx.ptr, ccall((:hank_primal, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, xhh, agg))
    het_keys = Tuple(Symbol.(vars_of_type(model, :heterogeneous)))
    if length(het_keys) == 1 && het_keys[1] == ctx.outputs[1]
        F = Array{Float64}(undef, P, P, n_hh); Dv = Matrix{Float64}(undef, P, n_hh)
        _check(ctx.ptr, ccall((:hank_fake_news, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, F, Dv))
        return _toeplitz_recursion(F, Dv)
    end
    n_het = _n_het(ctx, het_keys)
    Fh = Array{Float64}(undef, P, P, n_hh, n_het); Dvh = Array{Float64}(undef, P, n_hh, n_het)
    _check(ctx.ptr, ccall((:hank_fake_news_het, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}),
                          ctx.ptr, Int32(n_het), Fh, Dvh))
    return Dict(k => _toeplitz_recursion(Fh[:, :, :, o], Dvh[:, :, o]) for (k, o) in
                ((k, findfirst(==(k), ctx.outputs)) for k in het_keys))
end

# J[t, s] = J[t-1, s-1] + F[t, s], J[1, s] = Dv[s] + F[1, s] (:363-371), per household input k
function _toeplitz_recursion(F::Array{Float64,3}, Dv::Matrix{Float64})
    P, _, n_hh = size(F)
    J = similar(F)
    for k in 1:n_hh
        J[1, :, k] = Dv[:, k] .+ F[1, :, k]
        for t in 2:P
            J[t, 1, k] = F[t, 1, k]
            J[t, 2:P, k] = J[t-1, 1:P-1, k] .+ F[t, 2:P, k]
        end
    end
    return J
end

# ---- group outputs: aggregates by household group (hank_set_group_outputs, hank_get_group_outputs, hank_fake_news_group) -------
# W (G, K): one weight vector per group over the grid, indexed like D (vec of the (n_a, n_e) matrix), fixed over time; base[k] the
# policy it weighs: 0 mass (f = 1), 1 the policy variable a', 2 consumption. Y^k_t = sum W_k f D_t, dotted with the same D_t as
# every heterogeneous variable (ForwardIteration.jl:303-307). K = 0 (an empty W) clears the groups.
const HANK_GROUP_MASS, HANK_GROUP_POLICY, HANK_GROUP_CONS = Int32(0), Int32(1), Int32(2)
function hank_set_group_outputs(ctx::HankCtx, W::AbstractMatrix, base::AbstractVector{<:Integer})
    size(W, 2) == length(base) && (isempty(base) || size(W, 1) == ctx.G) || error("W must be (G, K) = ($(ctx.G), $(length(base)))")
    Wd = Matrix{Float64}(W); b = Vector{Int32}(base)
    _check(ctx.ptr, ccall((:hank_set_group_outputs, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}),
                          ctx.ptr, Int32(length(b)), isempty(b) ? C_NULL : Wd, isempty(b) ? C_NULL : b))
    ctx.n_groups = length(b)      # (after the check: a refused call leaves the library's set, and this count, as they were)
    return ctx
end

# agg (P, K) of the last primal, and with the dxhh (n_hh, P, N) of the last tangent sweep also dagg (P, K, N); the rules of
# hank_get_het_outputs (a batch with boundary seeds is refused)
function hank_get_group_outputs(ctx::HankCtx, dxhh::Union{Nothing,Array{Float64,3}} = nothing)
    K = max(ctx.n_groups, 1)      # (the library refuses a call without groups; the arrays are sized by the count it holds)
    agg = Matrix{Float64}(undef, ctx.P, K)
    N = dxhh === nothing ? 0 : size(dxhh, 3)
    dagg = dxhh === nothing ? nothing : Array{Float64}(undef, ctx.P, K, N)
    _check(ctx.ptr, ccall((:hank_get_group_outputs, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                          ctx.ptr, dxhh === nothing ? C_NULL : dxhh, Int32(N), agg, dagg === nothing ? C_NULL : dagg))
    return agg, dagg
end

# J[t, s, i] = d Y^k_t / d xhh_{i,s} per group k at the stationary primal the context holds (household_jacobian_toeplitz's
# precondition: hank_primal at the constant steady-state path), from the same recursion
function group_jacobian_toeplitz(ctx::HankCtx)
    P = ctx.P; n_hh = length(ctx.hh_rows); K = max(ctx.n_groups, 1)
    F = Array{Float64}(undef, P, P, n_hh, K); Dv = Array{Float64}(undef, P, n_hh, K)
    _check(ctx.ptr, ccall((:hank_fake_news_group, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx.ptr, F, Dv))
    return [_toeplitz_recursion(F[:, :, :, k], Dv[:, :, k]) for k in 1:K]
end

# ---- the transposed household block (hank_vjp) -----------------------------------------------------------------------------
# xhh_bar = J(x)' agg_bar at the primal the context has on record (the last hank_primal / hank_primal_jvp): the pullback of
# ForwardIteration (ForwardIteration.jl:339-420, on the reverse rule of transition_step, :131-192) followed by the transpose of
# the partials of BackwardIteration, for M cotangent columns at once. agg_bar is (P, n_het, M): cotangents of the aggregates of
# ctx.outputs[1] (the policy variable) and, with n_het = 2, of ctx.outputs[2] (consumption); xhh_bar is (n_hh, P, M), rows in
# the order of ctx.hh_rows. Returns xhh_bar.
function hank_vjp!(xhh_bar::Array{Float64,3}, ctx::HankCtx, agg_bar::Array{Float64,3})
    P, n_het, M = size(agg_bar)
    @assert P == ctx.P && size(xhh_bar) == (length(ctx.hh_rows), P, M)
    _check(ctx.ptr, ccall((:hank_vjp, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}),
                          ctx.ptr, Int32(n_het), agg_bar, Int32(M), xhh_bar))
    return xhh_bar
end

# hank_vjp! with cotangents on every heterogeneous output (hank_vjp_het): n_het up to length(ctx.outputs) — ctx.outputs[3], [4] are
# Value and UCE, which are not affine in the policy — and at most what hank_set_het_outputs declared. n_het <= 2: hank_vjp!'s bits.
function hank_vjp_het!(xhh_bar::Array{Float64,3}, ctx::HankCtx, agg_bar::Array{Float64,3})
    P, n_het, M = size(agg_bar)
    @assert P == ctx.P && size(xhh_bar) == (length(ctx.hh_rows), P, M)
    _check(ctx.ptr, ccall((:hank_vjp_het, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}),
                          ctx.ptr, Int32(n_het), agg_bar, Int32(M), xhh_bar))
    return xhh_bar
end

# ---- tangents and cotangents on the boundary (hank_jvp_boundary, hank_vjp_boundary) -----------------------------------------------
# dagg = the partials of the household block at the recorded primal for N directions seeded in the household inputs AND in
# `ss_end.value` (BackwardIteration.jl:85) AND in `ss_initial.D` (ForwardIteration.jl:293): dxhh (n_hh, P, N), dvalue_end and
# dD_init (n_a, n_e, N); `nothing` is a zero seed, at least one must be given. dagg is (P, N). Always the per-period launches.
# Afterwards hank_get_dpolicy_seq, hank_get_grid_aggregates and hank_get_het_outputs (n_het <= 2) serve this batch.
function hank_jvp_boundary!(dagg::Matrix{Float64}, ctx::HankCtx; dxhh::Union{Nothing,Array{Float64,3}} = nothing,
                            dvalue_end::Union{Nothing,Array{Float64,3}} = nothing, dD_init::Union{Nothing,Array{Float64,3}} = nothing)
    P, N = size(dagg)
    @assert P == ctx.P && !(dxhh === nothing && dvalue_end === nothing && dD_init === nothing)
    @assert dxhh === nothing || size(dxhh) == (length(ctx.hh_rows), P, N)
    @assert all(s -> s === nothing || size(s) == (ctx.n_a, ctx.n_e, N), (dvalue_end, dD_init))
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve dxhh dvalue_end dD_init begin
        _check(ctx.ptr, ccall((:hank_jvp_boundary, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}),
                              ctx.ptr, ptr(dxhh), ptr(dvalue_end), ptr(dD_init), Int32(N), dagg))
    end
    return dagg
end

# hank_vjp! with the cotangents of the boundary: value_end_bar and D_init_bar (n_a, n_e, M) receive the cotangents of
# `ss_end.value` and `ss_initial.D` (the reverse rules of ForwardIteration.jl:131-192, :339-420 carried through to
# ForwardIteration.jl:293, and the transpose of the backward loop through to BackwardIteration.jl:85); `nothing`: not wanted.
# n_het = size(agg_bar, 2) is 1 or 2; xhh_bar equals hank_vjp!'s bit for bit. Returns (xhh_bar, value_end_bar, D_init_bar).
function hank_vjp_boundary!(xhh_bar::Array{Float64,3}, value_end_bar::Union{Nothing,Array{Float64,3}}, D_init_bar::Union{Nothing,Array{Float64,3}},
                            ctx::HankCtx, agg_bar::Array{Float64,3})
    P, n_het, M = size(agg_bar)
    @assert P == ctx.P && size(xhh_bar) == (length(ctx.hh_rows), P, M)
    @assert all(s -> s === nothing || size(s) == (ctx.n_a, ctx.n_e, M), (value_end_bar, D_init_bar))
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve value_end_bar D_init_bar begin
        _check(ctx.ptr, ccall((:hank_vjp_boundary, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                              ctx.ptr, Int32(n_het), agg_bar, Int32(M), xhh_bar, ptr(value_end_bar), ptr(D_init_bar)))
    end
    return xhh_bar, value_end_bar, D_init_bar
end

# ---- every output's tangent in one pair of sweeps (hank_jvp_het) and its transpose on the boundary (hank_vjp_het_boundary) -------
# dagg (P, n_het, N), the shape of hank_get_het_outputs' tangents: n_het = size(dagg, 2) up to length(ctx.outputs) and at most what
# hank_set_het_outputs declared. Seeds as in hank_jvp_boundary!. Value and UCE (ctx.outputs[3], [4]) ride in the forward sweep, so
# the boundary's seeds reach them; n_het <= 2 gives the bits of hank_jvp / hank_jvp_boundary! on the per-period launches.
function hank_jvp_het!(dagg::Array{Float64,3}, ctx::HankCtx; dxhh::Union{Nothing,Array{Float64,3}} = nothing,
                       dvalue_end::Union{Nothing,Array{Float64,3}} = nothing, dD_init::Union{Nothing,Array{Float64,3}} = nothing)
    P, n_het, N = size(dagg)
    @assert P == ctx.P && !(dxhh === nothing && dvalue_end === nothing && dD_init === nothing)
    @assert dxhh === nothing || size(dxhh) == (length(ctx.hh_rows), P, N)
    @assert all(s -> s === nothing || size(s) == (ctx.n_a, ctx.n_e, N), (dvalue_end, dD_init))
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve dxhh dvalue_end dD_init begin
        _check(ctx.ptr, ccall((:hank_jvp_het, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}),
                              ctx.ptr, Int32(n_het), ptr(dxhh), ptr(dvalue_end), ptr(dD_init), Int32(N), dagg))
    end
    return dagg
end

# hank_vjp_boundary! with cotangents on every heterogeneous output (hank_vjp_het!'s rule for n_het = size(agg_bar, 2)): the exact
# transpose of hank_jvp_het!. xhh_bar equals hank_vjp_het!'s bit for bit. Returns (xhh_bar, value_end_bar, D_init_bar).
function hank_vjp_het_boundary!(xhh_bar::Array{Float64,3}, value_end_bar::Union{Nothing,Array{Float64,3}}, D_init_bar::Union{Nothing,Array{Float64,3}},
                                ctx::HankCtx, agg_bar::Array{Float64,3})
    P, n_het, M = size(agg_bar)
    @assert P == ctx.P && size(xhh_bar) == (length(ctx.hh_rows), P, M)
    @assert all(s -> s === nothing || size(s) == (ctx.n_a, ctx.n_e, M), (value_end_bar, D_init_bar))
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve value_end_bar D_init_bar begin
        _check(ctx.ptr, ccall((:hank_vjp_het_boundary, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                              ctx.ptr, Int32(n_het), agg_bar, Int32(M), xhh_bar, ptr(value_end_bar), ptr(D_init_bar)))
    end
    return xhh_bar, value_end_bar, D_init_bar
end

# hank_vjp_group: cotangents on the K group outputs of hank_set_group_outputs (grp_bar (P, K, M), the shape of
# hank_get_group_outputs' tangents) through the transposed sweeps — the exact transpose of hank_get_group_outputs' tangent map
# (ForwardIteration.jl:303-307 is the weighted dot, :339-420 the reverse rule). agg_bar (P, n_het, M), n_het 1 or 2, or nothing:
# cotangents on outputs 0 and 1 in the same product. value_end_bar, D_init_bar (n_a, n_e, M) or nothing (not wanted).
# Returns (xhh_bar, value_end_bar, D_init_bar).
function hank_vjp_group!(xhh_bar::Array{Float64,3}, ctx::HankCtx, grp_bar::Array{Float64,3}; agg_bar::Union{Nothing,Array{Float64,3}} = nothing,
                         value_end_bar::Union{Nothing,Array{Float64,3}} = nothing, D_init_bar::Union{Nothing,Array{Float64,3}} = nothing)
    P, K, M = size(grp_bar)
    @assert P == ctx.P && (ctx.n_groups == 0 || K == ctx.n_groups) && size(xhh_bar) == (length(ctx.hh_rows), P, M)
    @assert agg_bar === nothing || (size(agg_bar, 1) == P && size(agg_bar, 3) == M)
    @assert all(s -> s === nothing || size(s) == (ctx.n_a, ctx.n_e, M), (value_end_bar, D_init_bar))
    n_het = agg_bar === nothing ? 0 : size(agg_bar, 2)
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve agg_bar value_end_bar D_init_bar begin
        _check(ctx.ptr, ccall((:hank_vjp_group, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                              ctx.ptr, Int32(n_het), ptr(agg_bar), grp_bar, Int32(M), xhh_bar, ptr(value_end_bar), ptr(D_init_bar)))
    end
    return xhh_bar, value_end_bar, D_init_bar
end

# ---- derivatives through the steady state (hank_ss_jvp, hank_ss_vjp) ----------------------------------------------------------------
# What ForwardDiff.jacobian(F, p) carries through the VFI and invariant_dist inside find_ss (SteadyState.jl:195, :132-141;
# ForwardIteration.jl:446-530), from the record of hank_primal at the constant steady-state path with the steady state as both
# boundaries (hank_fake_news's precondition). dxhh (n_hh, N): directions in the household prices; dagg (n_het, N); dvalue, dpolicy,
# dD (n_a, n_e, N) or nothing (not wanted). Returns (dagg, iters, resid): steps and last increment ratio of the value and the
# distribution loop; a loop that ran into max_iter is an error here (the library reports it as HANK_OK, like hank_vfi).
function hank_ss_jvp!(dagg::Matrix{Float64}, ctx::HankCtx, dxhh::Matrix{Float64}; dvalue::Union{Nothing,Array{Float64,3}} = nothing,
                      dpolicy::Union{Nothing,Array{Float64,3}} = nothing, dD::Union{Nothing,Array{Float64,3}} = nothing,
                      tol::Float64 = 1e-13, max_iter::Integer = 50_000)
    n_het, N = size(dagg)
    @assert size(dxhh) == (length(ctx.hh_rows), N)
    @assert all(s -> s === nothing || size(s) == (ctx.n_a, ctx.n_e, N), (dvalue, dpolicy, dD))
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    iters, resid = zeros(Int32, 2), zeros(Float64, 2)
    GC.@preserve dvalue dpolicy dD begin
        _check(ctx.ptr, ccall((:hank_ss_jvp, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                                                            Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                              ctx.ptr, Int32(n_het), dxhh, Int32(N), tol, Int32(max_iter), ptr(dvalue), ptr(dpolicy), ptr(dD), dagg, iters, resid))
    end
    all(k -> iters[k] < max_iter || resid[k] <= tol, 1:2) || error("hank_ss_jvp: a loop took max_iter = $max_iter steps (increment ratios $resid)")
    return dagg, iters, resid
end

# The transpose: cotangents agg_bar (n_het, M) of the steady state's aggregates, value_bar and D_bar (n_a, n_e, M) of V_ss and D_ss
# (e.g. hank_vjp_het_boundary!'s value_end_bar), `nothing` where one is zero, not all three -> xhh_bar (n_hh, M).
function hank_ss_vjp!(xhh_bar::Matrix{Float64}, ctx::HankCtx; agg_bar::Union{Nothing,Matrix{Float64}} = nothing,
                      value_bar::Union{Nothing,Array{Float64,3}} = nothing, D_bar::Union{Nothing,Array{Float64,3}} = nothing,
                      n_het::Integer = agg_bar === nothing ? 1 : size(agg_bar, 1), tol::Float64 = 1e-13, max_iter::Integer = 50_000)
    M = size(xhh_bar, 2)
    @assert size(xhh_bar, 1) == length(ctx.hh_rows) && !(agg_bar === nothing && value_bar === nothing && D_bar === nothing)
    @assert agg_bar === nothing || size(agg_bar) == (n_het, M)
    @assert all(s -> s === nothing || size(s) == (ctx.n_a, ctx.n_e, M), (value_bar, D_bar))
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    iters, resid = zeros(Int32, 2), zeros(Float64, 2)
    GC.@preserve agg_bar value_bar D_bar begin
        _check(ctx.ptr, ccall((:hank_ss_vjp, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Int32, Ptr{Float64},
                                                            Ptr{Int32}, Ptr{Float64}),
                              ctx.ptr, Int32(n_het), ptr(agg_bar), ptr(value_bar), ptr(D_bar), Int32(M), tol, Int32(max_iter), xhh_bar, iters, resid))
    end
    all(k -> iters[k] < max_iter || resid[k] <= tol, 1:2) || error("hank_ss_vjp: a loop took max_iter = $max_iter steps (increment ratios $resid)")
    return xhh_bar, iters, resid
end

# ---- the household block at K input paths (hank_primal_batch) -----------------------------------------------------------------------
# fullFunction's household block (NewtonRaphson.jl:77-83) at K points through one chain of launches — what a step rule in place of
# the alphaUpdate stub (:117-120) evaluates. xhh (n_hh, P, K) -> aggs (P, n_het, K); policies (n_a, n_e, P, K) or nothing (not
# wanted). Returns (aggs, status): status[k] is scenario k's code (0 = ok); check = true turns the first failing scenario into an
# error, check = false returns the healthy scenarios' outputs with the codes. The context's recorded primal stays as it was.
function hank_primal_batch!(aggs::Array{Float64,3}, ctx::HankCtx, xhh::Array{Float64,3}; policies::Union{Nothing,Array{Float64,4}} = nothing,
                            check::Bool = true)
    P, n_het, K = size(aggs)
    @assert size(xhh) == (length(ctx.hh_rows), P, K) && P == ctx.P
    @assert policies === nothing || size(policies) == (ctx.n_a, ctx.n_e, P, K)
    status = zeros(Int32, K)
    rc = GC.@preserve policies ccall((:hank_primal_batch, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                                     ctx.ptr, Int32(n_het), xhh, Int32(K), aggs, policies === nothing ? Ptr{Float64}(C_NULL) : pointer(policies), status)
    (check || !any(!=(0), status)) && _check(ctx.ptr, rc)       # (a refusal of the call itself — no scenario's verdict — is always an error)
    return aggs, status
end

# ---- the steady state's household side at K price vectors (hank_ss_batch) -----------------------------------------------------------
# get_xVals' inner fixed point (SteadyState.jl:132-141), invariant_dist's (ForwardIteration.jl:436-442, by the power method) and
# the aggregation of the heterogeneous keys at K constant price vectors through one chain of launches — the columns of
# ForwardDiff.jacobian's finite-difference stand-in and the trials of a step rule for find_ss (:184-233). xhh (n_hh, K); value
# (n_a, n_e, K): in the starting values (ones in the reference), out the converged ones; D (G, K) or nothing: in the starts (positive,
# normalised), out the iterates at which the rule first held, NOT normalised; with D, aggs (n_het, K) is filled. Returns
# (aggs, value, policy, D, iters (2, K): value steps and distribution iterations, status). check as in hank_primal_batch!.
function hank_ss_batch!(value::Array{Float64,3}, ctx::HankCtx, xhh::Matrix{Float64}, vfi_tol::Float64; n_het::Integer = 1,
                        D::Union{Nothing,Matrix{Float64}} = nothing, vfi_max_iter::Integer = 10_000, dist_tol::Float64 = 1e-15,
                        dist_max_iter::Integer = 500_000, check_every::Integer = 25, check::Bool = true)
    K = size(xhh, 2)
    @assert size(xhh, 1) == length(ctx.hh_rows) && size(value) == (ctx.n_a, ctx.n_e, K)
    @assert D === nothing || size(D) == (ctx.n_a * ctx.n_e, K)
    policy = Array{Float64}(undef, ctx.n_a, ctx.n_e, K)
    aggs = D === nothing ? nothing : Array{Float64}(undef, n_het, K)
    iters, supnorm, status = zeros(Int32, 2, K), zeros(Float64, K), zeros(Int32, K)
    np(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    rc = GC.@preserve D aggs ccall((:hank_ss_batch, LIBHANK), Cint,
                                   (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Float64, Int32, Float64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                                    Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}),
                                   ctx.ptr, Int32(n_het), xhh, Int32(K), vfi_tol, Int32(vfi_max_iter), dist_tol, Int32(dist_max_iter), Int32(check_every),
                                   value, policy, np(D), np(aggs), iters, supnorm, status)
    (check || !any(!=(0), status)) && _check(ctx.ptr, rc)
    return aggs, value, policy, D, iters, status
end

# the cotangent of the policy sequence of the last hank_vjp! / hank_vjp_het!, (n_a, n_e, P, M): the reference's Δpolicy_seqs
# (ForwardIteration.jl:412-416) for the policy variable when n_het = 1
function hank_policy_cotangent_seq(ctx::HankCtx, M::Integer)
    out = Array{Float64}(undef, ctx.n_a, ctx.n_e, ctx.P, M)
    _check(ctx.ptr, ccall((:hank_get_policy_cotangent_seq, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), ctx.ptr, Int32(M), out))
    return out
end

# A ChainRules-shaped pullback of the device household block, for callers that differentiate a scalar of the path in reverse
# mode: `agg, pb = ForwardIteration_pullback(seqs, model, ss_initial)`; `pb(Δagg)` takes the cotangents of the aggregates as a
# NamedTuple keyed like `agg` (the shape of the reference's ForwardIteration_pullback argument, ForwardIteration.jl:387) and
# returns the cotangent of the household inputs as an (n_hh, P) matrix (rows: ctx.hh_rows) — the device sweeps BackwardIteration
# and ForwardIteration together, so the pullback covers both. Heterogeneous keys beyond consumption (Value, UCE) take hank_vjp_het!.
function ForwardIteration_pullback(seqs::DevicePolicySeqs, model::SequenceModel, ss_initial)
    agg = ForwardIteration(seqs, model, ss_initial)             # records the primal the pullback is taken at
    ctx = hank_context(model)
    het_keys = Tuple(Symbol.(vars_of_type(model, :heterogeneous)))
    n_het = _n_het(ctx, het_keys)
    function pullback(Δagg)
        agg_bar = zeros(Float64, ctx.P, n_het, 1)
        for k in het_keys
            agg_bar[:, findfirst(==(k), ctx.outputs), 1] .= Δagg[k]
        end
        xhh_bar = Array{Float64}(undef, length(ctx.hh_rows), ctx.P, 1)
        return (n_het > 2 ? hank_vjp_het! : hank_vjp!)(xhh_bar, ctx, agg_bar)[:, :, 1]
    end
    return agg, pullback
end

# ---- a path of the discount factor (hank_set_discount_path, hank_jvp_shock, hank_vjp_shock, hank_fake_news_shock) ----------------
# beta_t is the factor in period t's Euler equation, u'(c_t) = beta_t E_t[V_{t+1}] (KrusellSmith.jl:59-62 inside the loop of
# BackwardIteration.jl:90-113), t = 1 .. P; beta_P multiplies the expectation of the terminal value. The reference has no path: it
# reads beta from model.params. `nothing` returns the context to that constant. Like a new boundary, a new path drops the record.
function hank_set_discount_path(ctx::HankCtx, beta_t::Union{Nothing,AbstractVector{<:Real}})
    if beta_t === nothing
        _check(ctx.ptr, ccall((:hank_set_discount_path, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, C_NULL))
    else
        length(beta_t) == ctx.P || error("beta_t must have P = $(ctx.P) entries")
        b = Vector{Float64}(beta_t)
        _check(ctx.ptr, ccall((:hank_set_discount_path, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, b))
    end
    return ctx
end

# dagg (P, N) under directions dxhh (n_hh, P, N) in the household inputs and dbeta (P, N) in the path, either `nothing` (zeros), at
# the recorded primal; the batch is current afterwards as hank_jvp's is (beta has no direct term in any output: pass the same dxhh,
# or zeros, to hank_get_het_outputs / hank_get_group_outputs)
function hank_jvp_shock(ctx::HankCtx, dxhh::Union{Nothing,Array{Float64,3}}, dbeta::Union{Nothing,Matrix{Float64}})
    (dxhh === nothing && dbeta === nothing) && error("at least one of dxhh, dbeta must be given")
    N = dxhh === nothing ? size(dbeta, 2) : size(dxhh, 3)
    dagg = Matrix{Float64}(undef, ctx.P, N)
    _check(ctx.ptr, ccall((:hank_jvp_shock, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}),
                          ctx.ptr, dxhh === nothing ? C_NULL : dxhh, dbeta === nothing ? C_NULL : dbeta, Int32(N), dagg))
    return dagg
end

# hank_vjp_het! with the cotangent of the path: agg_bar (P, n_het, M) -> (xhh_bar (n_hh, P, M), beta_bar (P, M)); the exact
# transpose of hank_jvp_shock followed by hank_get_het_outputs
function hank_vjp_shock!(xhh_bar::Array{Float64,3}, beta_bar::Matrix{Float64}, ctx::HankCtx, agg_bar::Array{Float64,3})
    P, n_het, M = size(agg_bar)
    @assert P == ctx.P && size(xhh_bar) == (length(ctx.hh_rows), P, M) && size(beta_bar) == (P, M)
    _check(ctx.ptr, ccall((:hank_vjp_shock, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                          ctx.ptr, Int32(n_het), agg_bar, Int32(M), xhh_bar, beta_bar))
    return xhh_bar, beta_bar
end

# J[t, s, o] = d Y^o_t / d beta_s for the first n_het outputs at the stationary primal the context holds (household_jacobian_toeplitz's
# precondition, and no path set), from the recursion of SteadyStateJacobian.jl:363-371 with the input fixed to beta
function shock_jacobian_toeplitz(ctx::HankCtx, n_het::Integer)
    P = ctx.P
    F = Array{Float64}(undef, P, P, n_het); Dv = Matrix{Float64}(undef, P, n_het)
    _check(ctx.ptr, ccall((:hank_fake_news_shock, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), ctx.ptr, Int32(n_het), F, Dv))
    return _toeplitz_recursion(F, Dv)
end

# ---- a path of income by productivity state (hank_set_income_path, hank_jvp_income, hank_vjp_income, hank_fake_news_income) -------
# y[e, t] is the additive income of productivity state e in period t's budget, c + a' = (1 + r_t) a + w_t z_e + tr_t + y_t[e]
# (KrusellSmith.jl:59-62 and :66-80 inside the loop of BackwardIteration.jl:90-113). The reference has no such path: its income
# process is a constant of the model. `nothing` clears it. Like a new boundary, a new path drops the record; it excludes a
# discount-factor path.
function hank_set_income_path(ctx::HankCtx, y::Union{Nothing,AbstractMatrix{<:Real}})
    if y === nothing
        _check(ctx.ptr, ccall((:hank_set_income_path, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, C_NULL))
    else
        size(y) == (ctx.n_e, ctx.P) || error("y must be (n_e, P) = ($(ctx.n_e), $(ctx.P)), got $(size(y))")
        yy = Matrix{Float64}(y)
        _check(ctx.ptr, ccall((:hank_set_income_path, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, yy))
    end
    return ctx
end

# dagg (P, N) under directions dxhh (n_hh, P, N) in the household inputs and dy (n_e, P, N) in the path, either `nothing` (zeros),
# at the recorded primal; the batch is current afterwards as hank_jvp's is. y has a direct term in consumption: pass the same dy to
# hank_het_outputs_income.
function hank_jvp_income(ctx::HankCtx, dxhh::Union{Nothing,Array{Float64,3}}, dy::Union{Nothing,Array{Float64,3}})
    (dxhh === nothing && dy === nothing) && error("at least one of dxhh, dy must be given")
    N = dxhh === nothing ? size(dy, 3) : size(dxhh, 3)
    dxhh === nothing || size(dxhh) == (length(ctx.hh_rows), ctx.P, N) || error("dxhh must be (n_hh, P, N)")
    dy === nothing || size(dy) == (ctx.n_e, ctx.P, N) || error("dy must be (n_e, P, N) = ($(ctx.n_e), $(ctx.P), $N), got $(size(dy))")
    dagg = Matrix{Float64}(undef, ctx.P, N)
    _check(ctx.ptr, ccall((:hank_jvp_income, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}),
                          ctx.ptr, dxhh === nothing ? C_NULL : dxhh, dy === nothing ? C_NULL : dy, Int32(N), dagg))
    return dagg
end

# (agg (P, n_het), dagg (P, n_het, N)) for n_het <= 2 with the direct term of the income directions in consumption's tangent
# (dy `nothing`: the ones the current batch carries, if any)
function hank_het_outputs_income(ctx::HankCtx, n_het::Integer, dxhh::Array{Float64,3}, dy::Union{Nothing,Array{Float64,3}})
    N = size(dxhh, 3)
    size(dxhh) == (length(ctx.hh_rows), ctx.P, N) || error("dxhh must be (n_hh, P, N)")
    dy === nothing || size(dy) == (ctx.n_e, ctx.P, N) || error("dy must be (n_e, P, N) = ($(ctx.n_e), $(ctx.P), $N), got $(size(dy))")
    agg = Matrix{Float64}(undef, ctx.P, n_het); dagg = Array{Float64}(undef, ctx.P, n_het, N)
    _check(ctx.ptr, ccall((:hank_get_het_outputs_income, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                          ctx.ptr, Int32(n_het), dxhh, dy === nothing ? C_NULL : dy, Int32(N), agg, dagg))
    return agg, dagg
end

# hank_vjp! with the cotangent of the path: agg_bar (P, n_het, M), n_het 1 or 2 -> (xhh_bar (n_hh, P, M), y_bar (n_e, P, M)); the
# exact transpose of hank_jvp_income followed by hank_het_outputs_income
function hank_vjp_income!(xhh_bar::Array{Float64,3}, y_bar::Array{Float64,3}, ctx::HankCtx, agg_bar::Array{Float64,3})
    P, n_het, M = size(agg_bar)
    @assert P == ctx.P && size(xhh_bar) == (length(ctx.hh_rows), P, M) && size(y_bar) == (ctx.n_e, P, M)
    _check(ctx.ptr, ccall((:hank_vjp_income, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                          ctx.ptr, Int32(n_het), agg_bar, Int32(M), xhh_bar, y_bar))
    return xhh_bar, y_bar
end

# J[t, s, e, o] = d Y^o_t / d y_s[e] for the first n_het (1 or 2) outputs at the stationary primal the context holds
# (household_jacobian_toeplitz's precondition, and no path set), from the recursion of SteadyStateJacobian.jl:363-371 with the input
# fixed to y[e]
function income_jacobian_toeplitz(ctx::HankCtx, n_het::Integer)
    P, n_e = ctx.P, ctx.n_e
    F = Array{Float64}(undef, P, P, n_e, n_het); Dv = Array{Float64}(undef, P, n_e, n_het)
    _check(ctx.ptr, ccall((:hank_fake_news_income, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), ctx.ptr, Int32(n_het), F, Dv))
    J = Array{Float64}(undef, P, P, n_e, n_het)
    for o in 1:n_het
        J[:, :, :, o] = _toeplitz_recursion(F[:, :, :, o], Dv[:, :, o])
    end
    return J
end

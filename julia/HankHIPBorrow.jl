# HankHIPBorrow.jl — the ccall shims of include/hank_hip_borrow.h: a path of the borrowing limit in the household block.
# Include it after HankHIP.jl, whose LIBHANK, HankCtx, _check and _toeplitz_recursion it uses:
#     include("/path/to/repo/julia/HankHIP.jl"); include("/path/to/repo/julia/HankHIPBorrow.jl")

# ---- a path of the borrowing limit (hank_set_borrow_path, hank_jvp_borrow, hank_vjp_borrow, hank_fake_news_borrow) ----------------
# amin_t is the limit in period t's choice, a'_t = max(g_t, amin_t) (KrusellSmith.jl:76 inside the loop of BackwardIteration.jl:90-113),
# t = 1 .. P. The reference has no path: it reads borrow_cons from model.params (KrusellSmith.jl:52). `nothing` returns the context to
# that constant. Like a new boundary, a new path drops the record; it excludes the other two paths. THE KINK: with amin_t <= a_grid[1]
# the limit never binds through max (the grid's flat extrapolation does) and every partial in amin_t is an exact zero, so a grid that
# is to show a response carries points below the limit; with amin_t on a later grid point the derivative is the left one.
function hank_set_borrow_path(ctx::HankCtx, amin_t::Union{Nothing,AbstractVector{<:Real}})
    if amin_t === nothing
        _check(ctx.ptr, ccall((:hank_set_borrow_path, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, C_NULL))
    else
        length(amin_t) == ctx.P || error("amin_t must have P = $(ctx.P) entries")
        b = Vector{Float64}(amin_t)
        _check(ctx.ptr, ccall((:hank_set_borrow_path, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, b))
    end
    return ctx
end

# dagg (P, N) under directions dxhh (n_hh, P, N) in the household inputs and damin (P, N) in the path, either `nothing` (zeros), at
# the recorded primal; the batch is current afterwards as hank_jvp's is (the limit has no direct term in any output: pass the same
# dxhh, or zeros, to hank_get_het_outputs / hank_get_group_outputs)
function hank_jvp_borrow(ctx::HankCtx, dxhh::Union{Nothing,Array{Float64,3}}, damin::Union{Nothing,Matrix{Float64}})
    (dxhh === nothing && damin === nothing) && error("at least one of dxhh, damin must be given")
    N = dxhh === nothing ? size(damin, 2) : size(dxhh, 3)
    dagg = Matrix{Float64}(undef, ctx.P, N)
    _check(ctx.ptr, ccall((:hank_jvp_borrow, LIBHANK), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}),
                          ctx.ptr, dxhh === nothing ? C_NULL : dxhh, damin === nothing ? C_NULL : damin, Int32(N), dagg))
    return dagg
end

# hank_vjp_het! with the cotangent of the path: agg_bar (P, n_het, M) -> (xhh_bar (n_hh, P, M), amin_bar (P, M)); the exact
# transpose of hank_jvp_borrow followed by hank_get_het_outputs
function hank_vjp_borrow!(xhh_bar::Array{Float64,3}, amin_bar::Matrix{Float64}, ctx::HankCtx, agg_bar::Array{Float64,3})
    P, n_het, M = size(agg_bar)
    @assert P == ctx.P && size(xhh_bar) == (length(ctx.hh_rows), P, M) && size(amin_bar) == (P, M)
    _check(ctx.ptr, ccall((:hank_vjp_borrow, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                          ctx.ptr, Int32(n_het), agg_bar, Int32(M), xhh_bar, amin_bar))
    return xhh_bar, amin_bar
end

# J[t, s, o] = d Y^o_t / d amin_s for the first n_het outputs at the stationary primal the context holds (household_jacobian_toeplitz's
# precondition, and no path set), from the recursion of SteadyStateJacobian.jl:363-371 with the input fixed to the limit
function borrow_jacobian_toeplitz(ctx::HankCtx, n_het::Integer)
    P = ctx.P
    F = Array{Float64}(undef, P, P, n_het); Dv = Matrix{Float64}(undef, P, n_het)
    _check(ctx.ptr, ccall((:hank_fake_news_borrow, LIBHANK), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}), ctx.ptr, Int32(n_het), F, Dv))
    return _toeplitz_recursion(F, Dv)
end

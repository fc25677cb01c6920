# IBHip.jl -- the binding a maintainer of ImmersedBoundary.jl would add to run the per-partition
# residual hot path on MI355X through libibhip.so (C ABI: include/ibhip.h).
#
# It plugs into the reference's own hooks and nothing else:
#   * `conv_to_backend = IBHip.converter(dom)` (or `IBHip.hip`), `conv_from_backend = Array` in `dom(f, args...)`
#     and `impose_bc!` (/root/reference/src/ImmersedBoundary.jl:823-824, :846-855, :1202-1203);
#   * `ArrayBackends.to_backend(part, hip)` (src/arraybends.jl:14-77, registered for Partition at
#     src/ImmersedBoundary.jl:788) -- specialised here to upload ONCE and cache a native handle;
#   * Julia multiple dispatch on the operators (src/ImmersedBoundary.jl:873-1157): methods for
#     `HipPartition` + `HipArray` that `ccall` the library, including `divergent`, the tuple `face_gradient`, the
#     `Accumulator` call, `impose_bc!` and the domain call `dom(f, args...)` on device-resident arrays;
#   * `Base.Broadcast` on `HipArray`: every broadcast node (`+ - * / max min abs`, powers, exp/log/trig, clamp, ifelse,
#     comparisons to `HipArray{Bool}`, scalars, row vectors `u∞'`, `.=`, `.-=`, `@.`)
#     becomes one elementwise kernel (`ibh_ew_*`), so closures like test/advection.jl:67-83 run unchanged --
#     tests/test_gpu_broadcast.py runs exactly that expression tree through the same C entry points from Python.
#
# No KernelAbstractions, no CUDA.jl/AMDGPU.jl: device memory is owned by the library
# (ibh_malloc/ibh_free) behind `HipArray`.  There is no Julia runtime in the build container, so this
# file is written against the reference's sources and the C header but has never been executed; the same
# ABI is exercised from Python by tests/ (see INTEGRATION.md).
module IBHip

using ImmersedBoundary
import ImmersedBoundary: Partition, Boundary, Domain, Accumulator, at_owners, at_neighbors, at_faces, green_gauss,
    unsigned_green_gauss, cell_gradient, face_distance, owner_distance, neighbor_distance, face_gradient, MUSCL,
    divergent, impose_bc!
import ImmersedBoundary.CFD: JST_sensor
import ImmersedBoundary.ArrayBackends: to_backend
import ImmersedBoundary: CFD, Turbulence, Solver
import LinearAlgebra

const lib = get(ENV, "IBHIP_LIB", "libibhip")

@inline function check(rc::Cint)
    rc == 0 || error("libibhip: " * unsafe_string(ccall((:ibh_last_error, lib), Cstring, ())))
    nothing
end

init(device::Integer = 0) = check(ccall((:ibh_init, lib), Cint, (Cint,), device))

# ---------------------------------------------------------------------------------------------------
# device arrays (column-major like Julia's own arrays, so `(ncells, nvars)` maps 1:1 to the ABI's `ld`)
# ---------------------------------------------------------------------------------------------------
mutable struct HipArray{T, N} <: AbstractArray{T, N}
    ptr::Ptr{Cvoid}
    dims::NTuple{N, Int}
    parent::Any   # the array a column view aliases (kept alive), or nothing for an owning array
    function HipArray{T, N}(::UndefInitializer, dims::NTuple{N, Int}) where {T, N}
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ibh_malloc, lib), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), p, max(prod(dims), 1) * _esize(T)))
        a = new{T, N}(p[], dims, nothing)
        finalizer(x -> ccall((:ibh_free, lib), Cint, (Ptr{Cvoid},), x.ptr), a)
        a
    end
    # non-owning alias (no finalizer): `@view C[:, dim]`
    HipArray{T, N}(ptr::Ptr{Cvoid}, dims::NTuple{N, Int}, parent) where {T, N} = new{T, N}(ptr, dims, parent)
end
HipArray{T}(u::UndefInitializer, dims::Int...) where {T} = HipArray{T, length(dims)}(u, dims)
# HipArray{Bool}: the result of a comparison; stored as Float32 0 / 1, the value the broadcast kernels compute with
_esize(::Type{T}) where {T} = T === Bool ? sizeof(Float32) : sizeof(T)
Base.size(a::HipArray) = a.dims
Base.similar(a::HipArray{T}, ::Type{S}, dims::Dims) where {T, S} = HipArray{S, length(dims)}(undef, dims)
Base.getindex(::HipArray, i...) = error("scalar indexing of a HipArray; copy it back with Array(a)")
# columns of a column-major (n, nv) field are contiguous: `@view C[:, dim]` / `C[:, dim]` alias them
Base.view(a::HipArray{T, 2}, ::Colon, j::Integer) where {T} =
    HipArray{T, 1}(a.ptr + (j - 1) * size(a, 1) * _esize(T), (size(a, 1),), a)
Base.getindex(a::HipArray{T, 2}, ::Colon, j::Integer) where {T} = copy(view(a, :, j))

"`conv_to_backend`: host array -> device array."
function hip(a::Array{T, N}) where {T, N}
    d = HipArray{T, N}(undef, size(a))
    check(ccall((:ibh_h2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), d.ptr, a, sizeof(a)))
    d
end
function hip(a::Array{Bool, N}) where {N}
    d = HipArray{Bool, N}(undef, size(a))
    h = Float32.(a)
    check(ccall((:ibh_h2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), d.ptr, h, sizeof(h)))
    d
end
hip(a::AbstractArray) = hip(Array(a))
hip(a::HipArray) = a

function Base.Array(d::HipArray{Bool, N}) where {N}
    a = Array{Float32, N}(undef, d.dims)
    check(ccall((:ibh_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), a, d.ptr, sizeof(a)))
    a .!= 0
end

"`conv_from_backend`: device array -> host array."
function Base.Array(d::HipArray{T, N}) where {T, N}
    a = Array{T, N}(undef, d.dims)
    check(ccall((:ibh_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), a, d.ptr, sizeof(a)))
    a
end

ld(a::HipArray) = Int64(size(a, 1))
nv(a::HipArray) = Cint(length(a) ÷ max(size(a, 1), 1))

"The converter handed to `conv_to_backend`: callable like `hip`, and carries what `to_backend(::Partition, conv)` cannot
see in a `Partition` -- the mesh's block size (`dom.mesh.block_size`, src/mesher.jl:977), which switches the library's
block-structured fast path on (it still verifies every block against the face lists)."
struct HipConv
    block_size::Int
end
(c::HipConv)(a) = hip(a)
converter(dom::Domain) = HipConv(dom.mesh.block_size)

# ---------------------------------------------------------------------------------------------------
# Base.Broadcast: one elementwise kernel per node of the broadcast tree (include/ibhip.h, ibh_ew_*)
# ---------------------------------------------------------------------------------------------------
const EW_ADD, EW_SUB, EW_MUL, EW_DIV, EW_MAX, EW_MIN, EW_SUM = Cint.(0:6)
const EW_ABS, EW_NEG, EW_SQRT, EW_COPY = Cint.(16:19)
const EW_LT, EW_LE, EW_GT, EW_GE, EW_EQ, EW_NE, EW_AND, EW_OR, EW_POW, EW_COPYSIGN, EW_ATAN2, EW_BMUL = Cint.(64:75)
const EW_EXP, EW_EXP2, EW_LOG, EW_LOG2, EW_LOG10, EW_SIN, EW_COS, EW_TANH, EW_ATAN, EW_SIGN, EW_INV, EW_NOT, EW_POW0, EW_SQR, EW_CUBE, EW_INVSQR = Cint.(80:95)
const EW_CLAMP, EW_IFELSE = Cint(112), Cint(113)
const _binop = IdDict{Any, Cint}(+ => EW_ADD, - => EW_SUB, * => EW_MUL, / => EW_DIV, max => EW_MAX, min => EW_MIN,
    (<) => EW_LT, (<=) => EW_LE, (>) => EW_GT, (>=) => EW_GE, (==) => EW_EQ, (!=) => EW_NE, (&) => EW_AND,
    (|) => EW_OR, (^) => EW_POW, copysign => EW_COPYSIGN, atan => EW_ATAN2)
const _unop = IdDict{Any, Cint}(abs => EW_ABS, - => EW_NEG, sqrt => EW_SQRT, identity => EW_COPY, + => EW_COPY,
    exp => EW_EXP, exp2 => EW_EXP2, log => EW_LOG, log2 => EW_LOG2, log10 => EW_LOG10, sin => EW_SIN, cos => EW_COS,
    tanh => EW_TANH, atan => EW_ATAN, sign => EW_SIGN, inv => EW_INV, (!) => EW_NOT)
const _ternop = IdDict{Any, Cint}(clamp => EW_CLAMP, ifelse => EW_IFELSE)
# Base.literal_pow(^, x, Val(p)) -- what `x .^ 2` lowers to -- for the exponents it defines by products
const _litpow = Dict{Int, Cint}(0 => EW_POW0, 1 => EW_COPY, 2 => EW_SQR, 3 => EW_CUBE, -1 => EW_INV, -2 => EW_INVSQR)
const _cmps = (EW_LT, EW_LE, EW_GT, EW_GE, EW_EQ, EW_NE)

struct HipStyle <: Base.Broadcast.BroadcastStyle end
Base.Broadcast.BroadcastStyle(::Type{<:HipArray}) = HipStyle()
Base.Broadcast.BroadcastStyle(::HipStyle, ::Base.Broadcast.DefaultArrayStyle{0}) = HipStyle()   # scalars
_hostarray() = error("broadcast between a HipArray and a host array: convert it with IBHip.hip first")
# host row vectors `u∞'` (1 x nv) broadcast down the rows; so 2-D host operands enter HipStyle, and every one that is not
# a row vector is rejected by `_push!` / `_operand` / `_eval` below with the message above
Base.Broadcast.BroadcastStyle(::HipStyle, ::Base.Broadcast.DefaultArrayStyle{2}) = HipStyle()
const _HostRow = Union{LinearAlgebra.Adjoint{<:Real, <:AbstractVector}, LinearAlgebra.Transpose{<:Real, <:AbstractVector}}
Base.Broadcast.BroadcastStyle(::HipStyle, ::Base.Broadcast.BroadcastStyle) = _hostarray()

_rows(a::HipArray) = size(a, 1)
_operand(a::HipArray) = (a.ptr, nv(a), 0f0)
_operand(x::Number) = (C_NULL, Cint(0), Float32(x))
_operand(x::Base.RefValue) = _operand(x[])
_operand(x::AbstractArray) = _hostarray()

"Evaluate one node: operands are HipArrays (same shape, or a column vector over the columns) or scalars."
function _ew(op, a, b, out::Union{HipArray, Nothing} = nothing)
    code = get(_binop, op) do
        error("IBHip broadcast: unsupported binary operation $op")
    end
    arrs = filter(x -> x isa HipArray, (a, b))
    isempty(arrs) && return op(a, b)
    big = arrs[argmax(map(length, arrs))]
    o = isnothing(out) ? similar(big) : out
    (pa, na, sa), (pb, nb, sb) = _operand(a), _operand(b)
    check(ccall((:ibh_ew_binary, lib), Cint,
        (Cint, Int64, Cint, Ptr{Cvoid}, Cint, Cfloat, Ptr{Cvoid}, Cint, Cfloat, Ptr{Cvoid}),
        code, _rows(big), nv(big), pa, na, sa, pb, nb, sb, o.ptr))
    o
end
function _ew(op, a::HipArray, out::Union{HipArray, Nothing} = nothing)
    code = get(_unop, op) do
        error("IBHip broadcast: unsupported unary operation $op")
    end
    o = isnothing(out) ? similar(a) : out
    check(ccall((:ibh_ew_unary, lib), Cint, (Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), code, length(a), a.ptr, o.ptr))
    o
end

# recursive evaluation of a (possibly nested, `@.`-fused) Broadcasted tree; n-ary + * max min fold left like Julia does
# (`max.(a, b, 1f-7)` of the reference's MUSCL, src/ImmersedBoundary.jl:1113-1157)
_eval(x) = x
function _eval(bc::Base.Broadcast.Broadcasted)
    args = map(_eval, bc.args)
    any(x -> x isa AbstractArray && !(x isa Union{HipArray, _HostRow}), args) && _hostarray()
    _node(bc.f, args...)
end
_node(f, a) = a isa HipArray ? (_oldop(f, a) ? _ew(f, a) : _one(f, a)) : f(_unref(a))
_node(f, a, b) = any(x -> x isa HipArray, (a, b)) && !_oldop(f, a, b) ? _one(f, a, b) : _ew(f, a, b)
_node(f, a, b, c) = any(x -> x isa HipArray, (a, b, c)) ? _one(f, a, b, c) : f(_unref(a), _unref(b), _unref(c))
_node(f::typeof(Base.literal_pow), p, x, v) = x isa HipArray ? _one(f, p, x, v) : f(_unref(p), x, _unref(v))
_oldop(f, args...) = (length(args) == 1 ? haskey(_unop, f) && _unop[f] <= EW_COPY : haskey(_binop, f) && _binop[f] <= EW_MIN) &&
    all(x -> _eltype(x) !== Bool && !(x isa _HostRow), args)
"One node as a one-instruction ibh_ew_eval program: the same device code a fused tree runs, so the same bits."
function _one(f, args...)
    r = _fused(Base.Broadcast.Broadcasted{HipStyle}(f, args), nothing)
    isnothing(r) && error("IBHip broadcast: unsupported operation $f on $(map(typeof, args))")
    r
end
_node(f::Union{typeof(+), typeof(*), typeof(max), typeof(min)}, a, b, c, rest...) = _node(f, _node(f, a, b), c, rest...)
_node(f::Union{typeof(+), typeof(*), typeof(max), typeof(min)}, a, b, c) = _node(f, _node(f, a, b), c)

# ---- the whole (fused) Broadcasted tree as ONE launch: a postfix program for ibh_ew_eval (at most 48 instructions,
# 8 arrays, 8 scalars, stack depth 8); n-ary + and * fold left like Julia does.  `nothing` = does not fit / unsupported
# node: the caller falls back to the node-by-node evaluation above (same bits).
const EW_PUSH_ARRAY, EW_PUSH_SCALAR = Cint(32), Cint(33)
const EW_PUSH_ROW = Cint(34)
mutable struct _Prog
    code::Vector{Int32}
    arrs::Vector{HipArray}
    scal::Vector{Float32}
    row::Int   # length of a row-vector operand (0: none): the number of columns of the result
end
function _push!(P::_Prog, a::HipArray)
    k = findfirst(x -> x.ptr == a.ptr && size(x) == size(a), P.arrs)
    if isnothing(k)
        length(P.arrs) == 8 && return nothing
        push!(P.arrs, a)
        k = length(P.arrs)
    end
    push!(P.code, EW_PUSH_ARRAY | Int32((k - 1) << 8))
    1
end
function _push!(P::_Prog, x::Number)
    v = Float32(x)
    k = findfirst(y -> reinterpret(UInt32, y) == reinterpret(UInt32, v), P.scal)   # -0f0 is not 0f0
    if isnothing(k)
        length(P.scal) == 32 && return nothing
        push!(P.scal, v)
        k = length(P.scal)
    end
    push!(P.code, EW_PUSH_SCALAR | Int32((k - 1) << 8))
    1
end
function _push!(P::_Prog, x::_HostRow)   # `u∞'`: nv scalars, the one of column j in column j
    v = Float32.(vec(collect(x)))
    length(P.scal) + length(v) > 32 && return nothing
    push!(P.code, EW_PUSH_ROW | Int32(length(P.scal) << 8))
    append!(P.scal, v)
    P.row = length(v)
    1
end
_push!(P::_Prog, x::Base.RefValue) = _push!(P, x[])
_push!(P::_Prog, x::AbstractArray) = _hostarray()   # (HipArray and row vectors have their own methods)
_push!(P::_Prog, x) = nothing

# element types as Julia's broadcast sees them: Float32 arithmetic, Bool comparisons
_eltype(a::HipArray{T}) where {T} = T
_eltype(x::Number) = typeof(x)
_eltype(x::Base.RefValue) = _eltype(x[])
_eltype(x::_HostRow) = eltype(x)
_eltype(bc::Base.Broadcast.Broadcasted) = Base.Broadcast.combine_eltypes(bc.f, bc.args)
_eltype(x) = Any
_unref(x) = x isa Base.RefValue ? x[] : x
# the value of a subtree without device operands (`s > 0.1`, `M∞^2` for host numbers), computed on the host exactly as
# Julia does; `nothing` if the subtree reads a device array or a host array
_hostval(x::Number) = x
_hostval(x::Base.RefValue) = x[] isa Union{Number, Function, Val} ? x[] : nothing
function _hostval(bc::Base.Broadcast.Broadcasted)
    vals = map(_hostval, bc.args)
    (any(isnothing, vals) || !any(v -> v isa Number, vals)) && return nothing
    bc.f(vals...)
end
_hostval(x) = nothing

"`x OP s` for Float32 x and Float64 s, exactly as Julia compares them: one Float32 threshold with the same truth table."
function _exact_cmp(code::Cint, s::Float64)
    f = Float32(s)
    (isnan(s) || Float64(f) == s) && return code, f
    up, down = Float64(f) > s ? f : nextfloat(f), Float64(f) < s ? f : prevfloat(f)
    code in (EW_GT, EW_GE) && return EW_GT, down
    code in (EW_LT, EW_LE) && return EW_LT, up
    code == EW_EQ ? (EW_LT, -Inf32) : (EW_NE, NaN32)   # never equal / always different
end
const _flip = Dict(EW_LT => EW_GT, EW_LE => EW_GE, EW_GT => EW_LT, EW_GE => EW_LE, EW_EQ => EW_EQ, EW_NE => EW_NE)

function _push!(P::_Prog, bc::Base.Broadcast.Broadcasted)
    hv = _hostval(bc)
    isnothing(hv) || return _push!(P, hv)   # no device operand: one scalar (a Bool is 0 / 1)
    f, args = bc.f, bc.args
    if f === Base.literal_pow && length(args) == 3 && _unref(args[1]) === (^) && _unref(args[3]) isa Val
        p = typeof(_unref(args[3])).parameters[1]
        _eltype(args[2]) === Bool && throw(TypeError(:literal_pow, "a Float32 base", Float32, Bool))
        if haskey(_litpow, p)
            d = _push!(P, args[2])
            isnothing(d) && return nothing
            push!(P.code, _litpow[p])
            return d
        end
        f, args = (^), (args[2], Float32(p))   # any other integer exponent: Float32 ^, in double, rounded once
    end
    if length(args) == 1
        haskey(_unop, f) || return nothing
        isb = _eltype(args[1]) === Bool
        (f === (!)) == isb || f in (abs, identity, +) ||
            throw(TypeError(Symbol(f), "a Float32 operand (a Bool one only for !)", Float32, _eltype(args[1])))
        d = _push!(P, args[1])
        isnothing(d) && return nothing
        push!(P.code, _unop[f])
        return d
    end
    if length(args) == 3 && haskey(_ternop, f)
        f === ifelse && _eltype(args[1]) !== Bool && throw(TypeError(:ifelse, "a Bool condition", Bool, _eltype(args[1])))
        f === clamp && any(a -> _eltype(a) === Bool, args) && throw(TypeError(:clamp, "Float32 operands", Float32, Bool))
        depth = 0
        for (w, a) in enumerate(args)
            d = _push!(P, a)
            isnothing(d) && return nothing
            depth = max(depth, w - 1 + d)
        end
        push!(P.code, _ternop[f])
        return depth
    end
    (haskey(_binop, f) && (length(args) == 2 || f === (+) || f === (*) || f === max || f === min)) || return nothing
    code = _binop[f]
    if length(args) == 2
        ta, tb = _eltype(args[1]), _eltype(args[2])
        if code in _cmps   # a Float64 scalar (or host subtree) is compared exactly; at most one side is host-only here
            a, b = _hostval(args[1]), _hostval(args[2])
            b isa Float64 && ((code, t) = _exact_cmp(code, b); args = (args[1], t))
            a isa Float64 && ((code, t) = _exact_cmp(_flip[code], a); args = (args[2], t))
        elseif code in (EW_AND, EW_OR)
            (ta === Bool && tb === Bool) || throw(TypeError(Symbol(f), "Bool operands", Bool, ta === Bool ? tb : ta))
        elseif ta === Bool && tb === Bool
            throw(TypeError(Symbol(f), "at most one Bool operand (two Bools give Int)", Float32, Bool))
        elseif code == EW_MUL && (ta === Bool || tb === Bool)   # Bool * Float: the strong zero
            code, args = EW_BMUL, ta === Bool ? args : (args[2], args[1])
        elseif code in (EW_POW, EW_COPYSIGN, EW_ATAN2) && (ta === Bool || tb === Bool)
            throw(TypeError(Symbol(f), "Float32 operands", Float32, Bool))
        end
    end
    depth = _push!(P, args[1])
    isnothing(depth) && return nothing
    for a in args[2:end]
        d = _push!(P, a)
        isnothing(d) && return nothing
        depth = max(depth, 1 + d)
        push!(P.code, code)
    end
    depth
end
"Evaluate `bc` into `dest` (or a new array) with one `ibh_ew_eval`; `nothing` if the tree does not fit one program."
function _fused(bc::Base.Broadcast.Broadcasted, dest::Union{HipArray, Nothing})
    T = _eltype(bc)
    T === Bool || T <: AbstractFloat ||
        throw(TypeError(:broadcast, "a Float32 or Bool result (arithmetic between Bools gives Int)", Float32, T))
    P = _Prog(Int32[], HipArray[], Float32[], 0)
    depth = _push!(P, bc)
    (isnothing(depth) || depth > 8 || length(P.code) > 48 || isempty(P.arrs)) && return nothing
    big = P.arrs[argmax(map(length, P.arrs))]
    n, k = _rows(big), max(nv(big), P.row)
    all(a -> _rows(a) == n && (nv(a) == k || nv(a) == 1), P.arrs) || return nothing
    (P.row == 0 || P.row == k) || error("IBHip broadcast: a row vector of length $(P.row) over $k columns")
    # Float64 scalars are rounded to Float32 (the result stays Float32); comparisons give HipArray{Bool}
    o = isnothing(dest) ? HipArray{T === Bool ? Bool : Float32, k > 1 ? 2 : ndims(big)}(undef, k > 1 ? (n, k) : size(big)) : dest
    (size(o, 1) == n && nv(o) == k) || return nothing
    ptrs = Ptr{Cvoid}[a.ptr for a in P.arrs]
    nvs = Int32[nv(a) for a in P.arrs]
    GC.@preserve P ptrs nvs check(ccall((:ibh_ew_eval, lib), Cint,
        (Int64, Cint, Cint, Ptr{Int32}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Int32}, Cint, Ptr{Cfloat}, Ptr{Cvoid}),
        n, k, length(P.code), P.code, length(ptrs), ptrs, nvs, length(P.scal), P.scal, o.ptr))
    o
end

function Base.copy(bc::Base.Broadcast.Broadcasted{HipStyle})
    r = _fused(bc, nothing)
    isnothing(r) ? _eval(bc) : r
end
function Base.copyto!(dest::HipArray, bc::Base.Broadcast.Broadcasted{HipStyle})
    # `dest .= f.(dest, x)` / `dest .-= x`: one launch straight into dest (elementwise: dest may be an operand)
    isnothing(_fused(bc, dest)) || return dest
    if length(bc.args) == 2 && _oldop(bc.f, bc.args...)
        a, b = map(_eval, bc.args)
        _ew(bc.f, a, b, dest)
    else
        r = _eval(bc)
        r isa HipArray ? _ew(identity, r, dest) : fill!(dest, r)
    end
    dest
end
Base.copyto!(dest::HipArray, bc::Base.Broadcast.Broadcasted{<:Base.Broadcast.DefaultArrayStyle{0}}) = fill!(dest, bc[])
function Base.fill!(a::HipArray{Float32}, v)
    check(ccall((:ibh_ew_fill, lib), Cint, (Int64, Cfloat, Ptr{Cvoid}), length(a), Float32(v), a.ptr))
    a
end
Base.copy(a::HipArray) = _ew(identity, a)

function _reduce(code::Cint, a::HipArray{Float32})
    out = HipArray{Float32, 1}(undef, (1,))
    check(ccall((:ibh_ew_reduce, lib), Cint, (Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), code, length(a), a.ptr, out.ptr))
    Array(out)[1]
end
Base.maximum(a::HipArray{Float32}) = _reduce(EW_MAX, a)
Base.minimum(a::HipArray{Float32}) = _reduce(EW_MIN, a)
Base.sum(a::HipArray{Float32}) = _reduce(EW_SUM, a)
"`sum(a; dims = 2)` of an (n, nv) field: the columns added in order, one launch; the result is (n, 1) as in Julia.
`sum(a)` (no `dims`) stays the whole-array reduction."
function Base.sum(a::HipArray{Float32, 2}; dims = :)
    dims === (:) && return _reduce(EW_SUM, a)   # `sum(a)`: the whole array, as before
    dims == 2 || error("IBHip: sum(a; dims) supports dims = 2")
    o = HipArray{Float32, 2}(undef, (size(a, 1), 1))
    check(ccall((:ibh_ew_reduce_rows, lib), Cint, (Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}), size(a, 1), nv(a), a.ptr, o.ptr))
    o
end

# ---------------------------------------------------------------------------------------------------
# Partition on the device: to_backend(part, hip) uploads once (the reference re-uploads per call, :848)
# ---------------------------------------------------------------------------------------------------
mutable struct HipPartition{Ti, Tf}   # (mutable: the handle is released by a finalizer, SURVEY.md 8b)
    handle::Ptr{Cvoid}
    host::Partition{Ti, Tf}
    nc::Int
    nf::Vector{Int}
    spacing::HipArray{Tf, 2}
    centers::HipArray{Tf, 2}
end
Base.ndims(p::HipPartition) = size(p.centers, 2)

const _cache = IdDict{Any, Any}()

"Bucketed `Accumulator.stencils` (src/accumulator.jl:46-61) -> CSR (offsets, indices), 1-based."
function csr(acc, n::Int)
    lens = zeros(Int32, n)
    for (len, (rows, _, _)) in acc.stencils
        lens[rows] .= len
    end
    off = Int32[1; 1 .+ cumsum(lens)]
    idx = Vector{Int32}(undef, off[end] - 1)
    for (len, (rows, st, _)) in acc.stencils
        for (k, r) in enumerate(rows), j = 1:len
            idx[off[r] + j - 1] = st[j, k]
        end
    end
    off, idx
end

to_backend(part::Partition, ::typeof(hip)) = to_backend(part, HipConv(8))   # mesher.jl:977 default; verified by the library
function to_backend(part::Partition{Ti, Tf}, conv::HipConv) where {Ti, Tf}
    get!(_cache, part) do
        nd = ndims(part)
        nc = size(part.spacing, 1)
        owners = [Int32.(part.face_owners_neighbors[d][1]) for d = 1:nd]
        neighs = [Int32.(part.face_owners_neighbors[d][2]) for d = 1:nd]
        left = [csr(part.face_accumulators[(d, false)], nc) for d = 1:nd]
        right = [csr(part.face_accumulators[(d, true)], nc) for d = 1:nd]
        nf = Int32[length(o) for o in owners]
        ptrs(v) = Ptr{Int32}[pointer(x) for x in v]
        h = Ref{Ptr{Cvoid}}(C_NULL)
        loff, lidx = first.(left), last.(left)
        roff, ridx = first.(right), last.(right)
        domain = Int32.(part.domain)
        iid = Int32.(part.image_in_domain)
        GC.@preserve owners neighs loff lidx roff ridx domain iid begin
            check(ccall((:ibh_partition_create, lib), Cint,
                (Ptr{Ptr{Cvoid}}, Cint, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Int32},
                 Ptr{Ptr{Int32}}, Ptr{Ptr{Int32}}, Ptr{Ptr{Int32}}, Ptr{Ptr{Int32}}, Ptr{Ptr{Int32}}, Ptr{Ptr{Int32}},
                 Int32, Ptr{Int32}, Ptr{Int32}, Cint, Cint),
                h, nd, nc, Array(part.spacing), Array(part.centers), nf,
                ptrs(owners), ptrs(neighs), ptrs(loff), ptrs(lidx), ptrs(roff), ptrs(ridx),
                length(iid), iid, domain, conv.block_size, 1 #= Julia indices =#))
        end
        hp = HipPartition{Ti, Tf}(h[], part, nc, Int.(nf), hip(Array(part.spacing)), hip(Array(part.centers)))
        finalizer(x -> ccall((:ibh_partition_destroy, lib), Cint, (Ptr{Cvoid},), x.handle), hp)
        hp
    end
end

# ---------------------------------------------------------------------------------------------------
# operators: same names / arity / return shapes as src/ImmersedBoundary.jl:873-1157
# ---------------------------------------------------------------------------------------------------
out_like(u::HipArray{T, N}, n::Int) where {T, N} = HipArray{T, N}(undef, (n, size(u)[2:end]...))

for (jl, c) in ((:at_owners, :ibh_at_owners), (:at_neighbors, :ibh_at_neighbors), (:at_faces, :ibh_at_faces),
                (:face_gradient, :ibh_face_gradient))
    @eval function $jl(part::HipPartition, u::HipArray, dim::Int)
        out = out_like(u, part.nf[dim])
        check(ccall(($(QuoteNode(c)), lib), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64),
            part.handle, dim, u.ptr, nv(u), ld(u), out.ptr, ld(out)))
        out
    end
end

function cell_gradient(part::HipPartition, u::HipArray, dim::Int)
    out = out_like(u, part.nc)
    check(ccall((:ibh_cell_gradient, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64),
        part.handle, dim, u.ptr, nv(u), ld(u), out.ptr, ld(out)))
    out
end
# the tuple form (ImmersedBoundary.jl:980-988): all dimensions in one sweep per field (ibh_cell_gradient_nd); the
# gradients along dimension d are the columns (d-1)*nv+1 : d*nv of one (nc, nd*nv) buffer, returned as aliasing views
function cell_gradient(part::HipPartition, u::HipArray{Float32, N}) where {N}
    nd, n, k = ndims(part), part.nc, nv(u)
    buf = HipArray{Float32, 2}(undef, (n, nd * k))
    check(ccall((:ibh_cell_gradient_nd, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64),
        part.handle, u.ptr, k, ld(u), buf.ptr, n, C_NULL, 0))
    dims = N == 1 ? (n,) : (n, k)
    tuple((HipArray{Float32, N}(buf.ptr + (d - 1) * k * n * sizeof(Float32), dims, buf) for d = 1:nd)...)
end

function _gg(part::HipPartition, uf::HipArray, dim::Int, uns::Int)
    out = out_like(uf, part.nc)
    check(ccall((:ibh_green_gauss, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Cint),
        part.handle, dim, uf.ptr, nv(uf), ld(uf), out.ptr, ld(out), uns))
    out
end
green_gauss(part::HipPartition, uf::HipArray, dim::Int) = _gg(part, uf, dim, 0)
unsigned_green_gauss(part::HipPartition, uf::HipArray, dim::Int) = _gg(part, uf, dim, 1)

for (jl, c) in ((:face_distance, :ibh_face_distance), (:owner_distance, :ibh_owner_distance),
                (:neighbor_distance, :ibh_neighbor_distance))
    @eval function $jl(part::HipPartition{Ti, Tf}, dim::Int) where {Ti, Tf}
        out = HipArray{Tf, 1}(undef, (part.nf[dim],))
        check(ccall(($(QuoteNode(c)), lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), part.handle, dim, out.ptr))
        out
    end
end

function JST_sensor(part::HipPartition, p::HipArray, dim::Int = 0)
    out = out_like(p, part.nc)
    check(ccall((:ibh_jst_sensor, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64),
        part.handle, dim, p.ptr, nv(p), ld(p), out.ptr, ld(out)))
    out
end

function MUSCL(part::HipPartition, u::HipArray, δu::HipArray, dim::Int;
               D::Union{HipArray, Nothing} = nothing, high_order::Bool = false)
    uL, uR = out_like(u, part.nf[dim]), out_like(u, part.nf[dim])
    check(ccall((:ibh_muscl, lib), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        part.handle, dim, u.ptr, δu.ptr, nv(u), ld(u), isnothing(D) ? C_NULL : D.ptr, high_order, uL.ptr, uR.ptr, ld(uL)))
    (uL, uR)
end

"`divergent(part, uf::Tuple)` (:950-956): sum over dims of `green_gauss`, accumulated in place."
function divergent(part::HipPartition, uf::Tuple)
    r = green_gauss(part, uf[1], 1)
    for dim = 2:ndims(part)
        r .+= green_gauss(part, uf[dim], dim)
    end
    r
end

"`face_gradient(part, u, ∇u::Tuple, dim)` (:1051-1069): normal component from the face difference, the others from `at_faces(∇u[i])`."
face_gradient(part::HipPartition, u::HipArray, ∇u::Tuple, dim::Int) =
    tuple((i == dim ? face_gradient(part, u, dim) : at_faces(part, ∇u[i], dim) for i = 1:ndims(part))...)

# ---------------------------------------------------------------------------------------------------
# Accumulator on the device (src/accumulator.jl:78-130, defaults op = +, f = identity, Δ = false: the only form the
# reference's callers use) -- interpolators of `impose_bc!`, coarseners / prolongators of `multigrid`
# ---------------------------------------------------------------------------------------------------
mutable struct HipAccumulator
    handle::Ptr{Cvoid}
    n_output::Int
    n_input::Int
end

"Bucketed stencils + weights -> CSR with weights (1-based indices)."
function csr_weighted(acc::Accumulator)
    off, idx = csr(acc, acc.n_output)
    w = ones(Float32, length(idx))
    for (len, (rows, _, wt)) in acc.stencils
        isnothing(wt) && continue
        for (k, r) in enumerate(rows), j = 1:len
            w[off[r] + j - 1] = wt[j, k]
        end
    end
    off, idx, w
end

function to_backend(acc::Accumulator, ::Union{typeof(hip), HipConv})
    get!(_cache, acc) do
        off, idx, w = csr_weighted(acc)
        n_in = isempty(idx) ? 0 : Int(maximum(idx))
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ibh_acc_create, lib), Cint,
            (Ptr{Ptr{Cvoid}}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Cint),
            h, acc.n_output, n_in, off, idx, w, 1))
        a = HipAccumulator(h[], acc.n_output, n_in)
        finalizer(x -> ccall((:ibh_acc_destroy, lib), Cint, (Ptr{Cvoid},), x.handle), a)
        a
    end
end

"`out .+= acc(a .- b)` in one launch (the prolongation step of `FAS!`, src/solver.jl:76)."
function accumulate_diff_add!(out::HipArray, acc::HipAccumulator, a::HipArray, b::HipArray)
    check(ccall((:ibh_accumulate_diff_add, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64),
        acc.handle, a.ptr, b.ptr, nv(a), ld(a), out.ptr, ld(out)))
    out
end
function (acc::HipAccumulator)(v::HipArray)
    out = out_like(v, acc.n_output)
    check(ccall((:ibh_accumulate, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64),
        acc.handle, v.ptr, nv(v), ld(v), out.ptr, ld(out)))
    out
end

# ---------------------------------------------------------------------------------------------------
# impose_bc! on device-resident global arrays (src/ImmersedBoundary.jl:1197-1247): per boundary chunk
#   ia = W * a[image_domain]  (ibh_bc_interp),  ba = f(bdry, ia...),  a[ghost] = η ia + (1 - η) ba  (ibh_bc_blend)
# ---------------------------------------------------------------------------------------------------
mutable struct HipBoundary{Ti, Tf}
    handle::Ptr{Cvoid}
    host::Boundary{Ti, Tf}
    ng::Int
    projections::HipArray{Tf, 2}
    normals::HipArray{Tf, 2}
    image_distances::HipArray{Tf, 1}
    ghost_distances::HipArray{Tf, 1}
end

function to_backend(b::Boundary{Ti, Tf}, ::Union{typeof(hip), HipConv}) where {Ti, Tf}
    get!(_cache, b) do
        off, idx, w = csr_weighted(b.image_interpolator)
        gi, idm = Int32.(b.ghost_indices), Int32.(b.image_domain)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ibh_bc_create, lib), Cint,
            (Ptr{Ptr{Cvoid}}, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Int32, Ptr{Int32},
             Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Cint),
            h, length(gi), gi, Float32.(b.ghost_distances), Float32.(b.image_distances), length(idm), idm,
            off, idx, w, 1))
        hb = HipBoundary{Ti, Tf}(h[], b, length(gi), hip(Array(b.projections)), hip(Array(b.normals)),
                                 hip(Array(b.image_distances)), hip(Array(b.ghost_distances)))
        finalizer(x -> ccall((:ibh_bc_destroy, lib), Cint, (Ptr{Cvoid},), x.handle), hb)
        hb
    end
end

function impose_bc!(f, dom::Domain, bname::String, args::HipArray{Float32}...; kwargs...)
    for (_, b) in dom.boundaries[bname]
        bdry = to_backend(b, hip)
        iargs = map(args) do a
            ia = out_like(a, bdry.ng)
            check(ccall((:ibh_bc_interp, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64),
                bdry.handle, a.ptr, nv(a), ld(a), ia.ptr, ld(ia)))
            ia
        end
        r = f(bdry, iargs...; kwargs...)
        r isa Tuple || (r = (r,))
        for (a, ba, ia) in zip(args, r, iargs)
            if ba isa HipArray       # an array of boundary values, (ng,) broadcast over the columns or (ng, nv)
                bfull = size(ba) == size(ia) ? ba : ia .* 0f0 .+ ba
                check(ccall((:ibh_bc_blend, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cfloat}),
                    bdry.handle, a.ptr, nv(a), ld(a), ia.ptr, ld(ia), bfull.ptr, ld(bfull), C_NULL))
            else                     # a constant (per variable): the closure returned a number
                c = fill(Float32(ba), Int(nv(a)))
                check(ccall((:ibh_bc_blend, lib), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cfloat}),
                    bdry.handle, a.ptr, nv(a), ld(a), ia.ptr, ld(ia), C_NULL, 0, c))
            end
        end
    end
    nothing
end

# ---------------------------------------------------------------------------------------------------
# the domain call on device-resident global arrays (src/ImmersedBoundary.jl:820-864): one gather launch copies
# `a[part.domain]` of every argument and partition into stacked workspaces, `f` runs per partition on aliases of
# them, one scatter launch writes `a[part.image] .= local[part.image_in_domain]` -- snapshot semantics, the
# deterministic form of the reference's `tmap` (include/ibhip.h, ibh_domain_*)
# ---------------------------------------------------------------------------------------------------
mutable struct HipDomainPlan
    handle::Ptr{Cvoid}
    ids::Vector{Any}         # partition keys, in call order
    n::Vector{Int}           # rows of each partition (length(part.domain))
    ws_off::Vector{Int64}    # partition p's block of a field of nv variables starts at element nv * ws_off[p]
end

function domain_plan(dom::Domain)
    get!(_cache, (dom, :domain_plan)) do
        ids = collect(keys(dom.partitions))
        parts = [dom.partitions[i] for i in ids]
        doms = [Int32.(p.domain) for p in parts]
        imgs = [Int32.(p.image) for p in parts]
        iids = [Int32.(p.image_in_domain) for p in parts]
        nd = Int32[length(x) for x in doms]
        ni = Int32[length(x) for x in imgs]
        h = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve doms imgs iids begin
            check(ccall((:ibh_domain_plan_create, lib), Cint,
                (Ptr{Ptr{Cvoid}}, Cint, Ptr{Ptr{Int32}}, Ptr{Int32}, Ptr{Ptr{Int32}}, Ptr{Ptr{Int32}}, Ptr{Int32}, Int64,
                 Cint),
                h, length(ids), Ptr{Int32}[pointer(x) for x in doms], nd, Ptr{Int32}[pointer(x) for x in imgs],
                Ptr{Int32}[pointer(x) for x in iids], ni, length(dom), 1 #= Julia indices =#))
        end
        off = Vector{Int64}(undef, length(ids) + 1)
        check(ccall((:ibh_domain_plan_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Cint), h[], off, length(off)))
        pl = HipDomainPlan(h[], ids, Int.(nd), off)
        finalizer(x -> ccall((:ibh_domain_plan_destroy, lib), Cint, (Ptr{Cvoid},), x.handle), pl)
        pl
    end
end

# at least one positional HipArray: the zero-argument call stays the reference's method
function (dom::Domain)(f, a::HipArray{Float32}, args::HipArray{Float32}...;
                       conv_to_backend = nothing, conv_from_backend = nothing, n_threads::Int = 0, kwargs...)
    (isnothing(conv_to_backend) && isnothing(conv_from_backend)) ||
        error("domain call on HipArrays: no converters (the arrays are already on the device)")
    arrs = (a, args...)
    n = length(dom)
    for x in arrs
        size(x, 1) == n || throw(DimensionMismatch("domain call argument has $(size(x, 1)) rows, the domain $n cells"))
    end
    pl = domain_plan(dom)
    k = length(arrs)
    nvs = Cint[nv(x) for x in arrs]
    lds = Int64[ld(x) for x in arrs]
    ws = [HipArray{Float32, 1}(undef, (Int(nvs[j]) * Int(pl.ws_off[end]),)) for j = 1:k]
    check(ccall((:ibh_domain_gather, lib), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
        pl.handle, k, Ptr{Cvoid}[x.ptr for x in arrs], nvs, lds, Ptr{Cvoid}[w.ptr for w in ws]))
    conv = converter(dom)
    results = map(enumerate(pl.ids)) do (p, i)
        np = pl.n[p]
        locals = map(1:k) do j   # (n_p, nv...) column-major with ld = n_p: aliases of the workspace
            N = ndims(arrs[j])
            HipArray{Float32, N}(ws[j].ptr + Int(nvs[j]) * pl.ws_off[p] * sizeof(Float32),
                                 (np, size(arrs[j])[2:end]...), ws[j])
        end
        f(to_backend(dom.partitions[i], conv), locals...; kwargs...)
    end
    check(ccall((:ibh_domain_scatter, lib), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cint}, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
        pl.handle, k, Ptr{Cvoid}[w.ptr for w in ws], nvs, lds, Ptr{Cvoid}[x.ptr for x in arrs]))
    results
end

# ---------------------------------------------------------------------------------------------------
# fused residual sweeps (bypass broadcast: one C call = the whole closure of test/advection.jl:67-83)
# ---------------------------------------------------------------------------------------------------
"`ud .= -Σ_d green_gauss(upwind MUSCL/JST flux)`: the closure of test/advection.jl:67-83, fused."
function residual_advection!(ud::HipArray, part::HipPartition, u::HipArray, C::HipArray; flags::Integer = 0)
    check(ccall((:ibh_residual_advection, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint),
        part.handle, u.ptr, C.ptr, ld(C), ud.ptr, flags))
    ud
end

# layout of `ibh_fluid` (include/ibhip.h): R, gamma, mu_ref, Tref, S, nk, k[4]
struct IbhFluid
    R::Float32
    γ::Float32
    μref::Float32
    Tref::Float32
    S::Float32
    nk::Int32
    k::NTuple{4, Float32}
end
IbhFluid(fluid) = IbhFluid(fluid.R, fluid.γ, fluid.μref, fluid.Tref, fluid.S, Int32(min(length(fluid.k), 4)),
    ntuple(i -> i <= length(fluid.k) ? Float32(fluid.k[i]) : 0f0, 4))

"`R .= -Σ_d green_gauss(inviscid_fluxes(MUSCL(P)))` with the pressure JST sensor (CFD.inviscid_fluxes, cfd.jl:459)."
function residual_euler_hll!(R::HipArray, part::HipPartition, P::HipArray, fluid; flags::Integer = 0)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_residual_euler_hll, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{IbhFluid}, Cint),
        part.handle, P.ptr, ld(P), R.ptr, ld(R), f, flags))
    R
end

"The same closure with `CFD.inviscid_fluxes(fluid, PL, PR, at_owners(part, ν, dim), at_neighbors(part, ν, dim), dim)`
(cfd.jl:516): central flux + Rusanov dissipation scaled by the sensor `ν` (`nc` values), or by the pressure JST sensor when
`ν === nothing`."
function residual_euler_sensor!(R::HipArray, part::HipPartition, P::HipArray, fluid;
        ν::Union{HipArray, Nothing} = nothing, flags::Integer = 0)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_residual_euler_sensor, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{IbhFluid}, Cint),
        part.handle, P.ptr, ld(P), isnothing(ν) ? C_NULL : ν.ptr, R.ptr, ld(R), f, flags))
    R
end

# ---------------------------------------------------------------------------------------------------
# an explicit solver step, device resident: the body of `march!` (test/advection.jl:61-89)
# ---------------------------------------------------------------------------------------------------
"An ordered list of `impose_bc!` calls whose closures are `value` constants or `copy(u)` (test/advection.jl:30-46),
compiled once; `apply!(set, u)` has the semantics of the sequential calls."
mutable struct HipBCSet
    handle::Ptr{Cvoid}
    bcs::Vector{Any}          # keeps the HipBoundary structs alive
end
function HipBCSet(bcs::Vector, closures::Vector)   # closures[i] = :copy or a number
    modes = Int32[c === :copy ? 1 : 0 for c in closures]
    vals = Float32[c === :copy ? 0f0 : Float32(c) for c in closures]
    hs = Ptr{Cvoid}[b.handle for b in bcs]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve hs modes vals check(ccall((:ibh_bcset_create, lib), Cint,
        (Ptr{Ptr{Cvoid}}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Int32}, Ptr{Cfloat}), out, length(hs), hs, modes, vals))
    s = HipBCSet(out[], collect(Any, bcs))
    finalizer(x -> ccall((:ibh_bcset_destroy, lib), Cint, (Ptr{Cvoid},), x.handle), s)
    s
end
apply!(s::HipBCSet, u::HipArray{Float32}) = (check(ccall((:ibh_bcset_apply, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}),
    s.handle, u.ptr)); u)

"`dt = scale * 0.5 / maximum(max.(unsigned_green_gauss(at_faces(C_d, d), d)...))` (test/advection.jl:52-59, 65) left in
device memory (`dt::HipArray` of length 1)."
function timestep_advection!(dt::HipArray{Float32}, part::HipPartition, C::HipArray{Float32}; scale = 1f0)
    check(ccall((:ibh_timestep_advection, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cfloat, Ptr{Cvoid}),
        part.handle, C.ptr, ld(C), Float32(scale), dt.ptr))
    dt
end

"`u_out = u + dt * R(u)` (closure of test/advection.jl:67-83 + `u .+= ud .* dt`, :86) in one launch, then the BC set."
function step_advection!(u_out::HipArray{Float32}, part::HipPartition, u::HipArray{Float32}, C::HipArray{Float32},
                         dt::HipArray{Float32}, bcs::Union{HipBCSet, Nothing} = nothing)
    check(ccall((:ibh_step_advection, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
        part.handle, u.ptr, u_out.ptr, C.ptr, ld(C), dt.ptr, isnothing(bcs) ? C_NULL : bcs.handle))
    u_out
end

"The same step with `timestep_advection!(next_dt, part, C; scale)` for the NEXT step evaluated on the way (it depends on `C`
alone): extra workgroups of the BC set's own launches instead of two launches in front of the next sweep.  `next_dt` may be
`dt` itself."
function step_advection!(u_out::HipArray{Float32}, part::HipPartition, u::HipArray{Float32}, C::HipArray{Float32},
                         dt::HipArray{Float32}, bcs::Union{HipBCSet, Nothing}, next_dt::HipArray{Float32}; scale = 1f0)
    check(ccall((:ibh_step_advection_dt, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}),
        part.handle, u.ptr, u_out.ptr, C.ptr, ld(C), dt.ptr, isnothing(bcs) ? C_NULL : bcs.handle, Float32(scale), next_dt.ptr))
    u_out
end

# ---- an explicit Euler step, device resident (rows of P: [p T u v (w)])
"The CFL time step of an explicit Euler step: the formula of `timestep_advection!` with `C_d = abs.(u_d) .+ speed_of_sound`
evaluated from `P` on the fly.  `dt` (length 1) and / or `dt_cells` (length `nc`, the local time step) are written; returns
`dt` (or `dt_cells` when `dt === nothing`)."
function timestep_euler(part::HipPartition, P::HipArray{Float32}, fluid; scale = 1f0,
                        dt::Union{HipArray{Float32}, Nothing} = nothing, dt_cells::Union{HipArray{Float32}, Nothing} = nothing)
    isnothing(dt) && isnothing(dt_cells) && (dt = HipArray{Float32}(undef, 1))
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_timestep_euler, lib), Cint, (Ptr{Cvoid}, Ptr{IbhFluid}, Ptr{Cvoid}, Int64, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}),
        part.handle, f, P.ptr, ld(P), Float32(scale), isnothing(dt) ? C_NULL : dt.ptr, isnothing(dt_cells) ? C_NULL : dt_cells.ptr))
    isnothing(dt) ? dt_cells : dt
end

"`P_out = state2primitive(fluid, primitive2state(fluid, P) .+ dt .* R)` in one launch; `dt` of length 1, or one per row.
`P_out` may be `P`."
function update_euler!(P_out::HipArray{Float32}, fluid, P::HipArray{Float32}, R::HipArray{Float32}, dt::HipArray{Float32})
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_update_euler, lib), Cint,
        (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64),
        f, size(P, 2) - 2, size(P, 1), P.ptr, ld(P), R.ptr, ld(R), dt.ptr, length(dt) == 1 ? 0 : 1, P_out.ptr, ld(P_out)))
    P_out
end

"One explicit Euler step, `update_euler!(P_out, fluid, P, residual_euler_hll!/sensor!(work, part, P, fluid; flags), dt)`: one
launch where the 2-D single-kernel sweep takes the whole partition (global `dt`, `P_out !== P`), the sweep into `work` and the
update elsewhere (`work` is `nc × (nd + 2)` and must be given there).  `scheme`: `:hll` or `:sensor`."
function step_euler!(P_out::HipArray{Float32}, part::HipPartition, P::HipArray{Float32}, dt::HipArray{Float32}, fluid;
                     scheme::Symbol = :hll, work::Union{HipArray{Float32}, Nothing} = nothing, flags::Integer = 0)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_step_euler, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Cint),
        part.handle, f, scheme === :sensor ? 1 : 0, P.ptr, ld(P), P_out.ptr, ld(P_out), dt.ptr, length(dt) == 1 ? 0 : 1,
        isnothing(work) ? C_NULL : work.ptr, isnothing(work) ? 0 : ld(work), flags))
    P_out
end

"A Runge-Kutta stage of the low-storage family, `P_out = state2primitive(fluid, primitive2state(fluid, P0) .+ (alpha .* dt) .* R)`
in one launch, bit for bit `update_euler!(P_out, fluid, P0, R, dt .* Float32(alpha))`; `dt` of length 1, or one per row.
`P_out` may be `P0`."
function update_euler_stage!(P_out::HipArray{Float32}, fluid, P0::HipArray{Float32}, R::HipArray{Float32}, dt::HipArray{Float32},
                             alpha::Real)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_update_euler_stage, lib), Cint,
        (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Cfloat, Ptr{Cvoid}, Int64),
        f, size(P0, 2) - 2, size(P0, 1), P0.ptr, ld(P0), R.ptr, ld(R), dt.ptr, length(dt) == 1 ? 0 : 1, Float32(alpha), P_out.ptr,
        ld(P_out)))
    P_out
end

"One stage of a multi-stage step, `update_euler_stage!(P_out, fluid, P0, residual_euler_hll!/sensor!(work, part, P, fluid; flags),
dt, alpha)`: `P` is the previous stage, `P0` the state the step started from.  One launch where the 2-D single-kernel sweep
takes the whole partition and `P_out !== P` (with `dt` of length 1 or one per cell), the sweep into `work` and the update
elsewhere (`work` is `nc × (nd + 2)` and must be given there).  `P_out` may be `P0` when `P0 !== P`.  An `m`-stage step runs
this with `alpha = 1 / (m - k + 1)`, `k = 1:m`."
function stage_euler!(P_out::HipArray{Float32}, part::HipPartition, P::HipArray{Float32}, P0::HipArray{Float32},
                      dt::HipArray{Float32}, alpha::Real, fluid; scheme::Symbol = :hll,
                      work::Union{HipArray{Float32}, Nothing} = nothing, flags::Integer = 0)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_stage_euler, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Cfloat,
         Ptr{Cvoid}, Int64, Cint),
        part.handle, f, scheme === :sensor ? 1 : 0, P.ptr, ld(P), P0.ptr, ld(P0), P_out.ptr, ld(P_out), dt.ptr,
        length(dt) == 1 ? 0 : 1, Float32(alpha), isnothing(work) ? C_NULL : work.ptr, isnothing(work) ? 0 : ld(work), flags))
    P_out
end

"A Shu-Osher stage of a strong-stability-preserving Runge-Kutta scheme, `P_out = state2primitive(fluid, (primitive2state(fluid,
P0) .* a .+ primitive2state(fluid, P) .* b) .+ R .* (dt .* c))` in one launch, every product and sum rounded on its own; `dt` of
length 1, or one per row.  `P_out` may be `P0` or `P`."
function update_euler_ssp!(P_out::HipArray{Float32}, fluid, P0::HipArray{Float32}, P::HipArray{Float32}, R::HipArray{Float32},
                           dt::HipArray{Float32}, a::Real, b::Real, c::Real)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_update_euler_ssp, lib), Cint,
        (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Cfloat, Cfloat,
         Cfloat, Ptr{Cvoid}, Int64),
        f, size(P0, 2) - 2, size(P0, 1), P0.ptr, ld(P0), P.ptr, ld(P), R.ptr, ld(R), dt.ptr, length(dt) == 1 ? 0 : 1, Float32(a),
        Float32(b), Float32(c), P_out.ptr, ld(P_out)))
    P_out
end

"One Shu-Osher stage, `update_euler_ssp!(P_out, fluid, P0, P, residual_euler_hll!/sensor!(work, part, P, fluid; flags), dt, a, b,
c)`: `P` is the previous stage, `P0` the state the step started from.  One launch where the 2-D single-kernel sweep takes the
whole partition and `P_out !== P` (with `dt` of length 1 or one per cell), the sweep into `work` and the update elsewhere
(`work` is `nc × (nd + 2)` and must be given there).  `P_out` may be `P0` when `P0 !== P`.  SSPRK3 runs `stage_euler!` with
`alpha = 1` on `P0`, then this with `(3/4, 1/4, 1/4)` and `(1/3, 2/3, 2/3)`."
function stage_euler_ssp!(P_out::HipArray{Float32}, part::HipPartition, P::HipArray{Float32}, P0::HipArray{Float32},
                          dt::HipArray{Float32}, a::Real, b::Real, c::Real, fluid; scheme::Symbol = :hll,
                          work::Union{HipArray{Float32}, Nothing} = nothing, flags::Integer = 0)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_stage_euler_ssp, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Cfloat,
         Cfloat, Cfloat, Ptr{Cvoid}, Int64, Cint),
        part.handle, f, scheme === :sensor ? 1 : 0, P.ptr, ld(P), P0.ptr, ld(P0), P_out.ptr, ld(P_out), dt.ptr,
        length(dt) == 1 ? 0 : 1, Float32(a), Float32(b), Float32(c), isnothing(work) ? C_NULL : work.ptr,
        isnothing(work) ? 0 : ld(work), flags))
    P_out
end

"The source of a physical step of a dual time march, `S = primitive2state(fluid, Pn) .* cn .+ primitive2state(fluid, Pm) .* cm`
in one launch, or `primitive2state(fluid, Pn) .* cn` with `Pm = nothing` (BDF1, the first step).  BDF2 with the step `dt_real`:
`cn = 2 / dt_real`, `cm = -0.5 / dt_real`, and `g = 1.5 / dt_real` for the stages.  `S` aliases neither state."
function dual_source!(S::HipArray{Float32}, fluid, Pn::HipArray{Float32}, Pm::Union{HipArray{Float32}, Nothing}, cn::Real,
                      cm::Real)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_dual_source, lib), Cint,
        (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Cfloat, Cfloat, Ptr{Cvoid}, Int64),
        f, size(Pn, 2) - 2, size(Pn, 1), Pn.ptr, ld(Pn), isnothing(Pm) ? C_NULL : Pm.ptr, isnothing(Pm) ? 0 : ld(Pm), Float32(cn),
        Float32(cm), S.ptr, ld(S)))
    S
end

"A pseudo-time stage of a dual time step, `P_out = state2primitive(fluid, (primitive2state(fluid, P0) .+ (R .+ S) .* h) ./ (h .* g
.+ 1))` with `h = dt .* alpha` in one launch, every sum, product and the divide rounded on its own; `dt` of length 1, or one per
row.  `P_out` may be `P0`."
function update_euler_dual!(P_out::HipArray{Float32}, fluid, P0::HipArray{Float32}, R::HipArray{Float32}, S::HipArray{Float32},
                            dt::HipArray{Float32}, alpha::Real, g::Real)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_update_euler_dual, lib), Cint,
        (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Cfloat, Cfloat,
         Ptr{Cvoid}, Int64),
        f, size(P0, 2) - 2, size(P0, 1), P0.ptr, ld(P0), R.ptr, ld(R), S.ptr, ld(S), dt.ptr, length(dt) == 1 ? 0 : 1,
        Float32(alpha), Float32(g), P_out.ptr, ld(P_out)))
    P_out
end

"One pseudo-time stage of a dual time step, `update_euler_dual!(P_out, fluid, P0, residual_euler_hll!/sensor!(work, part, P, fluid;
flags), S, dt, alpha, g)`: `P` is the previous stage, `P0` the state the pseudo-step started from, `S` the source of the
physical step (`dual_source!`).  One launch where the 2-D single-kernel sweep takes the whole partition and `P_out !== P` (with
`dt` of length 1 or one per cell), the sweep into `work` and the update elsewhere (`work` is `nc × (nd + 2)` and must be given
there).  `P_out` may be `P0` when `P0 !== P`; `S` is neither `P_out` nor `work`."
function stage_euler_dual!(P_out::HipArray{Float32}, part::HipPartition, P::HipArray{Float32}, P0::HipArray{Float32},
                           S::HipArray{Float32}, dt::HipArray{Float32}, alpha::Real, g::Real, fluid; scheme::Symbol = :hll,
                           work::Union{HipArray{Float32}, Nothing} = nothing, flags::Integer = 0)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_stage_euler_dual, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid},
         Cint, Cfloat, Cfloat, Ptr{Cvoid}, Int64, Cint),
        part.handle, f, scheme === :sensor ? 1 : 0, P.ptr, ld(P), P0.ptr, ld(P0), S.ptr, ld(S), P_out.ptr, ld(P_out), dt.ptr,
        length(dt) == 1 ? 0 : 1, Float32(alpha), Float32(g), isnothing(work) ? C_NULL : work.ptr,
        isnothing(work) ? 0 : ld(work), flags))
    P_out
end

"The restriction of a multigrid cycle of the Euler march in conserved variables (not in ImmersedBoundary.jl), one launch:
`P_c = state2primitive(fluid, coarsener(primitive2state(fluid, P)))` and `D_c = coarsener(R .+ S)`, or `coarsener(R)` with
`S = nothing`, bit for bit those launches.  `coarsener`: `to_backend` of a coarsener of `multigrid(dom)`.  `P_c` and `D_c` alias
neither each other nor an input; the coarse forcing of the cycle is `D_c .- R_c(P_c)`."
function restrict_euler!(P_c::HipArray{Float32}, D_c::HipArray{Float32}, coarsener::HipAccumulator, fluid, P::HipArray{Float32},
                         R::HipArray{Float32}, S::Union{HipArray{Float32}, Nothing} = nothing)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_restrict_euler, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid},
         Int64),
        coarsener.handle, f, size(P, 2) - 2, P.ptr, ld(P), R.ptr, ld(R), isnothing(S) ? C_NULL : S.ptr, isnothing(S) ? 0 : ld(S),
        P_c.ptr, ld(P_c), D_c.ptr, ld(D_c)))
    P_c, D_c
end

"Cell roles of an immersed-boundary march, one `UInt8` per row (`cell_roles` of the Python package builds them on the host)."
const ROLE_FLUID, ROLE_GHOST, ROLE_SOLID = 0x00, 0x01, 0x02

"`restrict_euler!` with cell roles: `D_c = coarsener(t)` with `t = R .+ S` (or `R`) in the rows whose role is `ROLE_FLUID` and `+0`
in every other one -- a select, so a NaN in a masked row never reaches `D_c`; `P_c` is `restrict_euler!`'s.  One launch."
function restrict_euler_roles!(P_c::HipArray{Float32}, D_c::HipArray{Float32}, coarsener::HipAccumulator, fluid,
                               P::HipArray{Float32}, R::HipArray{Float32}, S::Union{HipArray{Float32}, Nothing},
                               roles::HipArray{UInt8})
    length(roles) == size(P, 1) || error("restrict_euler_roles!: one role per fine row")
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_restrict_euler_roles, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64,
         Ptr{Cvoid}, Int64),
        coarsener.handle, f, size(P, 2) - 2, P.ptr, ld(P), R.ptr, ld(R), isnothing(S) ? C_NULL : S.ptr, isnothing(S) ? 0 : ld(S),
        roles.ptr, P_c.ptr, ld(P_c), D_c.ptr, ld(D_c)))
    P_c, D_c
end

"The coarse forcing of a cycle with cell roles, in place and in one launch: `D .= D .- R` in the rows whose role is `ROLE_FLUID`,
`+0` in every other one.  At most 8 columns; `D` aliases neither `R` nor `roles`."
function forcing_roles!(D::HipArray{Float32}, R::HipArray{Float32}, roles::HipArray{UInt8})
    size(D) == size(R) && length(roles) == size(D, 1) || error("forcing_roles!: D and R of one shape, one role per row")
    check(ccall((:ibh_forcing_roles, lib), Cint, (Int64, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
        size(D, 1), size(D, 2), D.ptr, ld(D), R.ptr, ld(R), roles.ptr))
    D
end

"Per column of `x` (at most 8) the sum of squares over the rows whose role is `ROLE_FLUID`, in `Float64` on the device: `out`
holds `size(x, 2)` values and is assigned.  One launch for all columns and the one-launch final stage of the sums."
function sumsq_roles!(out::HipArray{Float64}, x::HipArray{Float32}, roles::HipArray{UInt8})
    length(out) == size(x, 2) && length(roles) == size(x, 1) || error("sumsq_roles!: one output per column, one role per row")
    check(ccall((:ibh_sumsq_roles, lib), Cint, (Int64, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
        size(x, 1), size(x, 2), x.ptr, ld(x), roles.ptr, out.ptr))
    out
end

"The prolongation of a multigrid cycle of the Euler march: `P_out = state2primitive(fluid, primitive2state(fluid, P) .+
prolongator(primitive2state(fluid, Pc_new) .- primitive2state(fluid, Pc_old)))` in two launches, bit for bit `primitive2state`
three times, `accumulate_diff_add!` and `state2primitive`.  `pack`: `8 * n_input` Float32 of scratch on the device, 32-byte
aligned (a `HipArray` is); `Pc_new` and `Pc_old` share their leading dimension.  `P_out` may be `P`."
function prolong_euler!(P_out::HipArray{Float32}, prolongator::HipAccumulator, fluid, P::HipArray{Float32},
                        Pc_new::HipArray{Float32}, Pc_old::HipArray{Float32}, pack::HipArray{Float32})
    ld(Pc_new) == ld(Pc_old) || error("prolong_euler!: Pc_new and Pc_old must share their leading dimension")
    length(pack) >= 8 * prolongator.n_input || error("prolong_euler!: pack holds fewer than 8 * n_input elements")
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_prolong_euler, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64),
        prolongator.handle, f, size(P, 2) - 2, Pc_new.ptr, Pc_old.ptr, ld(Pc_new), pack.ptr, P.ptr, ld(P), P_out.ptr,
        ld(P_out)))
    P_out
end

"Implicit residual smoothing (not in ImmersedBoundary.jl): `n_iter` Jacobi iterations on `(I + eps L) S = R`, `L` the unweighted
Laplacian of the partition's face graph, `S_i = (R_i + eps * Σ_f S[across(f, i)]) / (1 + eps * n_i)` from `S = R`, per column of
`R` (at most 8), one launch each.  The result lands in `S`; `tmp`, its ping-pong partner, is required from `n_iter = 2`.  `S` and
`tmp` alias neither each other nor `R`."
function smooth_residual!(S::HipArray{Float32}, part::HipPartition, R::HipArray{Float32}, eps::Real, n_iter::Integer;
                          tmp::Union{HipArray{Float32}, Nothing} = nothing)
    check(ccall((:ibh_smooth_residual, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cfloat, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64),
        part.handle, R.ptr, size(R, 2), ld(R), Float32(eps), n_iter, S.ptr, ld(S), isnothing(tmp) ? C_NULL : tmp.ptr,
        isnothing(tmp) ? 0 : ld(tmp)))
    S
end

"The last iteration of a residual smoothing inside the update, in one launch: with `S` one iteration of `smooth_residual!` from
`Sprev` (which may be `R`: the only iteration), `coef = (c,)` is `update_euler_stage!(P_out, fluid, P0, S, dt, c)` (`P` is
ignored and may be `nothing`) and `coef = (a, b, c)` is `update_euler_ssp!(P_out, fluid, P0, P, S, dt, a, b, c)`, bit for bit and
without `S` being written.  `P_out` may be `P0` or `P`, not `R` or `Sprev`."
function update_euler_smoothed!(P_out::HipArray{Float32}, part::HipPartition, fluid, P0::HipArray{Float32},
                                P::Union{HipArray{Float32}, Nothing}, R::HipArray{Float32}, Sprev::HipArray{Float32}, eps::Real,
                                dt::HipArray{Float32}, coef::Tuple)
    blend = length(coef) == 3
    a, b, c = blend ? coef : (0, 1, coef[1])
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_update_euler_smoothed, lib), Cint,
        (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Cfloat,
         Ptr{Cvoid}, Cint, Cfloat, Cfloat, Cfloat, Ptr{Cvoid}, Int64),
        part.handle, f, blend ? 1 : 0, P0.ptr, ld(P0), isnothing(P) ? C_NULL : P.ptr, isnothing(P) ? 0 : ld(P), R.ptr, ld(R),
        Sprev.ptr, ld(Sprev), Float32(eps), dt.ptr, length(dt) == 1 ? 0 : 1, Float32(a), Float32(b), Float32(c), P_out.ptr,
        ld(P_out)))
    P_out
end

"`S .+ Σ_d green_gauss(at_faces(ν .+ νR, d) .* face_gradient(R, d) .- at_faces(vel[:, d] .* R, d), d)` in one launch
(the transport residual closed by `Wray_Agarwal`, src/turbulence.jl:222-241), bit-identical to the composition."
function scalar_transport!(out::HipArray{Float32}, part::HipPartition, R::HipArray{Float32}, νR::HipArray{Float32},
                           ν::Real, vel::HipArray{Float32}, S::HipArray{Float32})
    check(ccall((:ibh_scalar_transport, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
        part.handle, R.ptr, νR.ptr, Float32(ν), vel.ptr, ld(vel), S.ptr, out.ptr))
    out
end

"`shear_rate([cell_gradient(part, vel[:, i]) for i in 1:nd])` (src/turbulence.jl:110-124) in one launch where the partition
is made of complete 3-D blocks or has no block structure (an error otherwise: compose the operators)."
function shear_rate_of_velocity!(S::HipArray{Float32}, part::HipPartition, vel::HipArray{Float32})
    check(ccall((:ibh_shear_rate_of_velocity, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
        part.handle, vel.ptr, ld(vel), S.ptr))
    S
end

"The same with the velocity gradients kept: `G` is `(nc, nd * nd)`, `∂u_i/∂x_j` in column `nd (j - 1) + i` -- the tuple
`cell_gradient(part, vel)` is the column blocks `G[:, nd (j - 1) + 1 : nd j]` -- for `viscous_residual!` (the gradients of a
Navier-Stokes closure with a turbulence model are made once)."
function shear_rate_of_velocity!(S::HipArray{Float32}, G::HipArray{Float32, 2}, part::HipPartition, vel::HipArray{Float32})
    check(ccall((:ibh_shear_rate_of_velocity_grad, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        part.handle, vel.ptr, ld(vel), S.ptr, G.ptr, ld(G)))
    S, G
end

"The LES closure of a velocity field in one launch, the gradients `g[i][j] = cell_gradient(part, vel[:, i])[j]` consumed where
they are made (same partitions as `shear_rate_of_velocity!`): any of `νSGS` (`model = :smagorinsky`:
`Smagorinsky_νSGS(Δ, shear_rate(g); Cs)`, src/turbulence.jl:134-137; `model = :wale`: `WALE_νSGS(Δ, g; Cw)`, :292-337, 3-D
only), `ducros = Ducros_sensor(g)` (:253-283), `shock = CFD.shock_sensor(g)` (src/cfd.jl:589-617), `S = shear_rate(g)`
(:110-124) and `G`, the gradients in the layout of `shear_rate_of_velocity!`.  Outputs left `nothing` are not written."
function les_closure_of!(part::HipPartition, vel::HipArray{Float32}; Δ = nothing, model = nothing, Cs = 0.17f0,
                         Cw = 0.325f0, νSGS = nothing, ducros = nothing, shock = nothing, S = nothing, G = nothing)
    m = isnothing(model) ? 0 : model == :smagorinsky ? 1 : model == :wale ? 2 :
        error("les_closure_of!: model must be nothing, :smagorinsky or :wale")
    p(a) = isnothing(a) ? C_NULL : a.ptr
    check(ccall((:ibh_les_of, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Cint, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        part.handle, vel.ptr, ld(vel), p(Δ), Cint(m), Float32(m == 1 ? Cs : Cw), p(νSGS), p(ducros), p(shock), p(S), p(G),
        isnothing(G) ? Int64(0) : ld(G)))
    (νSGS = νSGS, ducros = ducros, shock = shock, S = S, gradients = G)
end

"The right-hand sides of the standard k-ϵ model (src/turbulence.jl:175-194) in one launch (same partitions as
`shear_rate_of_velocity!`): `rk = Sk + transport(k; ν + νk)` and `rϵ = Sϵ + transport(ϵ; ν + νϵ)` with
`(νk, νϵ, Sk, Sϵ, νₜ) = standard_kϵ(k, ϵ, shear_rate(g))`, `g[i][j] = cell_gradient(part, vel[:, i])[j]`; `νₜ`, `S` and the
gradients `G` (layout of `shear_rate_of_velocity!`) are written when given."
function k_epsilon_rhs!(rk::HipArray{Float32}, rϵ::HipArray{Float32}, part::HipPartition, vel::HipArray{Float32},
                        k::HipArray{Float32}, ϵ::HipArray{Float32}, ν::Real; Cμ::Real = 0.09f0, σk::Real = 1.0f0,
                        σϵ::Real = 1.3f0, C1ϵ::Real = 1.44f0, C2ϵ::Real = 1.92f0, νₜ = nothing, S = nothing, G = nothing)
    p(a) = isnothing(a) ? C_NULL : a.ptr
    par = Float32[Cμ, σk, σϵ, C1ϵ, C2ϵ]
    check(ccall((:ibh_k_epsilon_rhs, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        part.handle, vel.ptr, ld(vel), k.ptr, ϵ.ptr, Float32(ν), par, rk.ptr, rϵ.ptr, p(νₜ), p(S), p(G),
        isnothing(G) ? Int64(0) : ld(G)))
    (rk = rk, rϵ = rϵ, νₜ = νₜ, S = S, gradients = G)
end

"`Wray_Agarwal(R, S, cell_gradient(part, R), cell_gradient(part, S))` (src/turbulence.jl:222-241) in one launch; returns
`(νt = nut, νR = nuR, S = Sout)` written into the three arrays."
function wray_agarwal_of!(nut::HipArray{Float32}, nuR::HipArray{Float32}, Sout::HipArray{Float32}, part::HipPartition,
                          R::HipArray{Float32}, S::HipArray{Float32}; σR = 0.72f0, C1 = 0.0829f0, κ = 0.41f0)
    check(ccall((:ibh_wray_agarwal_of, lib), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Cfloat, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        part.handle, R.ptr, S.ptr, Float32(σR), Float32(C1), Float32(κ), nut.ptr, nuR.ptr, Sout.ptr))
    (νt = nut, νR = nuR, S = Sout)
end

# flags of the fused sweeps (include/ibhip.h)
const FORCE_GENERAL, IMAGE_ONLY, PASS_A_ONLY, PASS_B_ONLY, EXACT = 1, 2, 4, 8, 16
const PHASE_INTERIOR, PHASE_BOUNDARY, NO_FUSE, NO_QUAD = 32, 64, 128, 1024

# ---------------------------------------------------------------------------------------------------
# point-implicit smoother: the device kernels behind src/point_implicit.jl (hutchinson_trick :17-91,
# _inverse_blocks! :124-135, PIPreconditioner :141-161, proj_along / solve :221-329).  A maintainer adds
# methods of those functions for HipArray that call these; the Python mirror of this repo
# (immersedboundary.jl_amd/point_implicit.py) shows the composition one to one.
# ---------------------------------------------------------------------------------------------------
"`D .= pinv` of every `nv x nv` block of `D::(n, nv, nv)`, or `1 ./ (eps .+ D)` for a vector (:124-135)."
function inverse_blocks!(D::HipArray{Float32})
    n = size(D, 1); nv = ndims(D) == 1 ? 1 : size(D, 2)
    check(ccall((:ibh_pi_invert_blocks, lib), Cint, (Int64, Cint, Ptr{Cvoid}), n, nv, D.ptr))
    D
end

"`out[p, k] = Σ_i v[p, i] * invD[p, k, i]` (:153-161)."
function apply_blocks!(out::HipArray{Float32}, invD::HipArray{Float32}, v::HipArray{Float32})
    n = size(v, 1); nv = ndims(v) == 1 ? 1 : size(v, 2)
    check(ccall((:ibh_pi_apply_blocks, lib), Cint, (Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        n, nv, invD.ptr, v.ptr, out.ptr))
    out
end

"`s[p, k] += z[p] * (fxb[p, k] - fx[p, k]) / h`: one Hutchinson sample (:40)."
function hutch_accum!(s::HipArray{Float32}, fxb::HipArray{Float32}, fx::HipArray{Float32}, z::HipArray{Float32}, h)
    n = size(s, 1); nv = ndims(s) == 1 ? 1 : size(s, 2)
    check(ccall((:ibh_pi_hutch_accum, lib), Cint, (Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}),
        n, nv, fxb.ptr, fx.ptr, z.ptr, Float32(h), s.ptr))
    s
end

"`out = x + v*h` (:30, :112) and `out = (fxb - fx)/h` (:110-114)."
perturb!(out::HipArray{Float32}, x::HipArray{Float32}, v::HipArray{Float32}, h) = (check(ccall((:ibh_pi_perturb, lib), Cint,
    (Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}), length(x), x.ptr, v.ptr, Float32(h), out.ptr)); out)
fd!(out::HipArray{Float32}, fxb::HipArray{Float32}, fx::HipArray{Float32}, h) = (check(ccall((:ibh_pi_fd, lib), Cint,
    (Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}), length(fx), fxb.ptr, fx.ptr, Float32(h), out.ptr)); out)

"`x .+= s .* α; r .-= As .* α` with `α = dots[1] / (dots[2] + eps)` read on the device (:229-236, :291-294)."
function relax_update!(x::HipArray{Float32}, r::HipArray{Float32}, s::HipArray{Float32}, As::HipArray{Float32},
                       dots::Ptr{Cvoid})
    check(ccall((:ibh_pi_update, lib), Cint, (Int64, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        length(r), dots, eps(Float32), s.ptr, As.ptr, x.ptr, r.ptr))
    nothing
end


# ---------------------------------------------------------------------------------------------------
# CFD pointwise physics on device arrays: methods of the reference's own functions (src/cfd.jl) for HipArray, so that a
# residual closure written against `CFD.*` runs unchanged after `conv_to_backend` (configs[1]-[4]).  Cartesian `dim` only
# (the matrix-normal forms of `inviscid_fluxes` / `viscous_fluxes` are a curvilinear extension outside this hot path).
# ---------------------------------------------------------------------------------------------------
_vec_like(a::HipArray{Float32}) = HipArray{Float32, ndims(a)}(undef, size(a))
for (jl, c) in ((:speed_of_sound, :ibh_cfd_speed_of_sound), (:dynamic_viscosity, :ibh_cfd_dynamic_viscosity),
                (:heat_conductivity, :ibh_cfd_heat_conductivity))
    @eval function CFD.$jl(fluid::CFD.Fluid, T::HipArray{Float32})   # cfd.jl:62-64, 71-77, 84-90
        out = _vec_like(T)
        f = Ref(IbhFluid(fluid))
        check(ccall(($(QuoteNode(c)), lib), Cint, (Ptr{IbhFluid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}), f, length(T), T.ptr, out.ptr))
        out
    end
end
_ndP(P::HipArray{Float32, 2}) = size(P, 2) - 2
function CFD.primitive2state(fluid::CFD.Fluid, P::HipArray{Float32, 2})   # cfd.jl:106-123
    Q = _vec_like(P)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_cfd_primitive2state, lib), Cint, (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64),
        f, _ndP(P), size(P, 1), P.ptr, ld(P), Q.ptr, ld(Q)))
    Q
end
function CFD.state2primitive(fluid::CFD.Fluid, Q::HipArray{Float32, 2})   # cfd.jl:137-151
    P = _vec_like(Q)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_cfd_state2primitive, lib), Cint, (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64),
        f, _ndP(Q), size(Q, 1), Q.ptr, ld(Q), P.ptr, ld(P)))
    P
end
function CFD.inviscid_fluxes(fluid::CFD.Fluid, PL::HipArray{Float32, 2}, PR::HipArray{Float32, 2}, dim::Integer)   # :459-508
    F = _vec_like(PL)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_cfd_inviscid_fluxes_hll, lib), Cint,
        (Ptr{IbhFluid}, Cint, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64),
        f, _ndP(PL), dim, size(PL, 1), PL.ptr, PR.ptr, ld(PL), F.ptr, ld(F)))
    F
end
function CFD.inviscid_fluxes(fluid::CFD.Fluid, PL::HipArray{Float32, 2}, PR::HipArray{Float32, 2},
                             νL::HipArray{Float32, 1}, νR::HipArray{Float32, 1}, dim::Integer)                     # :516-554
    F = _vec_like(PL)
    f = Ref(IbhFluid(fluid))
    check(ccall((:ibh_cfd_inviscid_fluxes_sensor, lib), Cint,
        (Ptr{IbhFluid}, Cint, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        f, _ndP(PL), dim, size(PL, 1), PL.ptr, PR.ptr, ld(PL), νL.ptr, νR.ptr, F.ptr, ld(F)))
    F
end
"`viscous_fluxes(fluid, P, Pgrad, dim; μₜ)` (cfd.jl:664-736): `Pgrad` a tuple / vector of the gradients of P along each axis."
function CFD.viscous_fluxes(fluid::CFD.Fluid, P::HipArray{Float32, 2}, Pgrad::Union{AbstractVector, Tuple}, dim::Integer;
                            μₜ::Union{HipArray{Float32, 1}, Real} = 0.0f0)
    F = _vec_like(P)
    f = Ref(IbhFluid(fluid))
    g = Ptr{Cvoid}[x.ptr for x in Pgrad]
    GC.@preserve g Pgrad begin
        check(ccall((:ibh_cfd_viscous_fluxes, lib), Cint,
            (Ptr{IbhFluid}, Cint, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Ptr{Cvoid}}, Int64, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}, Int64),
            f, _ndP(P), dim, size(P, 1), P.ptr, ld(P), g, ld(Pgrad[1]),
            μₜ isa HipArray ? μₜ.ptr : C_NULL, μₜ isa HipArray ? 0f0 : Float32(μₜ), F.ptr, ld(F)))
    end
    F
end
"`R[:, 2:end] .+= Σ_d green_gauss(part, viscous_fluxes(fluid, at_faces(part, P, d), face_gradient(part, P, ∇P, d), d; μₜ = at_faces(part, μₜ, d)), d)`
in one launch, bit-identical to that composition (`∇P = cell_gradient(part, P)`)."
function viscous_residual!(R::HipArray{Float32, 2}, part::HipPartition, fluid::CFD.Fluid, P::HipArray{Float32, 2}, ∇P::Tuple,
                           μₜ::HipArray{Float32, 1})
    f = Ref(IbhFluid(fluid))
    g = Ptr{Cvoid}[x.ptr for x in ∇P]
    GC.@preserve g ∇P begin
        check(ccall((:ibh_viscous_residual, lib), Cint,
            (Ptr{Cvoid}, Ptr{IbhFluid}, Ptr{Cvoid}, Int64, Ptr{Ptr{Cvoid}}, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
            part.handle, f, P.ptr, ld(P), g, ld(∇P[1]), size(∇P[1], 2) == size(P, 2) ? 2 : 0, μₜ.ptr, R.ptr, ld(R)))
    end
    R
end
"`(bc::FlowBC)(P, normals; image_distances, du!dn, transpiration)` (cfd.jl:243-300) on image-point arrays of a `HipBoundary`."
function (bc::CFD.FlowBC)(P::HipArray{Float32, 2}, normals::HipArray{Float32, 2};
                          image_distances::Union{Nothing, HipArray{Float32, 1}} = nothing,
                          du!dn::Union{Nothing, HipArray{Float32, 1}} = nothing,
                          transpiration::Union{Real, HipArray{Float32, 1}} = 0.0f0)
    isnothing(du!dn) == isnothing(image_distances) ||
        throw(error("du!dn and image_distances must be passed together for BC imposition"))
    out = _vec_like(P)
    f = Ref(IbhFluid(bc.fluid))
    u∞ = Float32.(collect(bc.u∞))
    check(ccall((:ibh_cfd_flow_bc, lib), Cint,
        (Ptr{IbhFluid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Cfloat, Cfloat, Ptr{Float32}, Cint, Ptr{Cvoid},
         Ptr{Cvoid}, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Int64),
        f, _ndP(P), size(P, 1), P.ptr, ld(P), normals.ptr, ld(normals), Float32(bc.p∞), Float32(bc.T∞), u∞,
        bc.normal_flow ? 1 : 0, isnothing(image_distances) ? C_NULL : image_distances.ptr,
        isnothing(du!dn) ? C_NULL : du!dn.ptr, transpiration isa Real ? Float32(transpiration) : 0f0,
        transpiration isa HipArray ? transpiration.ptr : C_NULL, out.ptr, ld(out)))
    out
end

# ---------------------------------------------------------------------------------------------------
# Turbulence closures (src/turbulence.jl) on device arrays.  Velocity gradients: the reference's Matrix of vectors,
# `velocity_gradient[i, j]` = ∂u_i/∂x_j -> an nd x nd table of device pointers, row-major g[(i-1) nd + j].
# ---------------------------------------------------------------------------------------------------
function _grad_table(g::AbstractMatrix)
    nd = size(g, 1)
    nd, Ptr{Cvoid}[g[i, j].ptr for i = 1:nd for j = 1:nd]
end
_wall_params(κ, C, A, β, βstar, D, A⁺, ω) = Float32[κ, C, A, β, βstar, D, A⁺, ω]
function Turbulence.wall_function(y::HipArray{Float32, 1}, u::HipArray{Float32, 1}, ν::HipArray{Float32, 1};
                                  κ::Real = 0.41f0, C::Real = 4.9f0, A::Real = 19.0f0, β::Real = 0.075f0,
                                  βstar::Real = 0.09f0, D::Real = 4.2f0, A⁺::Real = 360.0f0,
                                  ω_fixed_point::Real = 0.5f0, n_iter::Int = 20)                    # turbulence.jl:72-98
    o = ntuple(_ -> _vec_like(y), 6)
    par = _wall_params(κ, C, A, β, βstar, D, A⁺, ω_fixed_point)
    check(ccall((:ibh_turb_wall_function, lib), Cint,
        (Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Ptr{Cvoid}, Ptr{Cvoid}),
        length(y), y.ptr, u.ptr, ν.ptr, par, n_iter, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, o[5].ptr, o[6].ptr))
    (uτ = o[1], νₜ = o[2], k = o[3], ω = o[4], ϵ = o[5], du!dn = o[6])
end
function Turbulence.wall_function(Rey::HipArray{Float32, 1};
                                  κ::Real = 0.41f0, C::Real = 4.9f0, A::Real = 19.0f0, β::Real = 0.075f0,
                                  βstar::Real = 0.09f0, D::Real = 4.2f0, A⁺::Real = 360.0f0,
                                  ω_fixed_point::Real = 0.5f0, n_iter::Int = 20)                    # turbulence.jl:27-70
    o = ntuple(_ -> _vec_like(Rey), 5)
    par = _wall_params(κ, C, A, β, βstar, D, A⁺, ω_fixed_point)
    check(ccall((:ibh_turb_wall_function_rey, lib), Cint,
        (Int64, Ptr{Cvoid}, Ptr{Float32}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        length(Rey), Rey.ptr, par, n_iter, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, o[5].ptr))
    (y⁺ = o[1], u⁺ = o[2], μ⁺ = o[3], k⁺ = o[4], du⁺!dy⁺ = o[5])
end

# layout of `ibh_flow_bc_spec` (include/ibhip.h)
struct IbhFlowBCSpec
    normal_flow::Int32
    p∞::Float32
    T∞::Float32
    u∞::NTuple{3, Float32}
    transpiration::Float32
    wall_function::Int32
    wall_params::NTuple{8, Float32}
    n_iter::Int32
end
const _flow_bc_scalar_modes = Dict(:copy => Int32(1), :νₜ => Int32(2), :k => Int32(3), :ω => Int32(4), :ϵ => Int32(5))
"""
`impose_flow_bc!(dom, bname, bc, P, scalars...; wall_function = nothing, transpiration = 0)`: `impose_bc!` with the `FlowBC`
`bc` as its closure in one launch per boundary chunk (`ibh_bc_flow`) -- bit-identical to `impose_bc!` over `bc(Pi, b.normals;
du!dn, image_distances, transpiration)` with `du!dn` from `wall_function(b.image_distances, uₜ, μ(T) / ρ; wall_function...)` at
the image points where `wall_function` is a NamedTuple of its keywords (`(;)` for the defaults).  `scalars`: up to four pairs
`field => value` with a number, `:copy`, or -- with `wall_function` -- `:νₜ`, `:k`, `:ω`, `:ϵ`.
"""
function impose_flow_bc!(dom::Domain, bname::String, bc::CFD.FlowBC, P::HipArray{Float32, 2},
                         scalars::Pair{<:HipArray{Float32, 1}}...; wall_function::Union{Nothing, NamedTuple} = nothing,
                         transpiration::Real = 0f0)
    nd = _ndP(P)
    ns = length(scalars)
    ns <= 4 || throw(ArgumentError("impose_flow_bc!: at most 4 scalar fields"))
    u∞ = Float32.(collect(bc.u∞))
    bc.normal_flow && length(u∞) != 1 &&
        throw(ArgumentError("Only 3 parcels in P (p, T and normal flow) allowed for normal_flow = true BC"))
    wf = isnothing(wall_function) ? (;) : wall_function
    kw = merge((κ = 0.41f0, C = 4.9f0, A = 19.0f0, β = 0.075f0, βstar = 0.09f0, D = 4.2f0, A⁺ = 360.0f0,
                ω_fixed_point = 0.5f0, n_iter = 20), wf)
    par = _wall_params(kw.κ, kw.C, kw.A, kw.β, kw.βstar, kw.D, kw.A⁺, kw.ω_fixed_point)
    spec = Ref(IbhFlowBCSpec(bc.normal_flow ? 1 : 0, Float32(bc.p∞), Float32(bc.T∞),
                             ntuple(i -> i <= length(u∞) ? u∞[i] : 0f0, 3), Float32(transpiration),
                             isnothing(wall_function) ? 0 : 1, ntuple(i -> par[i], 8), Int32(kw.n_iter)))
    modes = Int32[v isa Symbol ? _flow_bc_scalar_modes[v] : Int32(0) for (_, v) in scalars]
    values = Float32[v isa Symbol ? 0f0 : Float32(v) for (_, v) in scalars]
    any(m >= 2 for m in modes) && isnothing(wall_function) &&
        throw(ArgumentError("impose_flow_bc!: :νₜ, :k, :ω and :ϵ need wall_function"))
    fields = Ptr{Cvoid}[a.ptr for (a, _) in scalars]
    f = Ref(IbhFluid(bc.fluid))
    for (_, b) in dom.boundaries[bname]
        bdry = to_backend(b, hip)
        direct = Ref{Int32}(0)
        check(ccall((:ibh_bc_flow_info, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}), bdry.handle, direct))
        staging = direct[] != 0 ? nothing : HipArray{Float32, 1}(undef, (bdry.ng * (nd + 2 + ns),))
        GC.@preserve fields scalars staging begin
            check(ccall((:ibh_bc_flow, lib), Cint,
                (Ptr{Cvoid}, Ptr{IbhFluid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{IbhFlowBCSpec}, Cint,
                 Ptr{Ptr{Cvoid}}, Ptr{Int32}, Ptr{Float32}, Ptr{Cvoid}),
                bdry.handle, f, nd, bdry.normals.ptr, ld(bdry.normals), bdry.image_distances.ptr, P.ptr, ld(P), spec, ns,
                fields, modes, values, isnothing(staging) ? C_NULL : staging.ptr))
        end
    end
    nothing
end
function Turbulence.shear_rate(velocity_gradient::AbstractMatrix{<:HipArray})                       # :110-124
    nd, tab = _grad_table(velocity_gradient)
    S = _vec_like(velocity_gradient[1, 1])
    GC.@preserve tab velocity_gradient check(ccall((:ibh_turb_shear_rate, lib), Cint,
        (Cint, Int64, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}), nd, length(S), tab, S.ptr))
    S
end
function Turbulence.Smagorinsky_νSGS(Δ::HipArray{Float32, 1}, S::HipArray{Float32, 1}; Cₛ::Real = 0.17f0)   # :134-138
    out = _vec_like(S)
    check(ccall((:ibh_turb_smagorinsky, lib), Cint, (Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cfloat, Ptr{Cvoid}),
        length(S), Δ.ptr, S.ptr, Float32(Cₛ), out.ptr))
    out
end
function Turbulence.standard_kϵ(k::HipArray{Float32, 1}, ϵ::HipArray{Float32, 1}, S::HipArray{Float32, 1};
                                Cμ::Real = 0.09f0, σk::Real = 1.0f0, σϵ::Real = 1.3f0, C1ϵ::Real = 1.44f0,
                                C2ϵ::Real = 1.92f0)                                                 # :175-196
    o = ntuple(_ -> _vec_like(k), 5)
    par = Float32[Cμ, σk, σϵ, C1ϵ, C2ϵ]
    check(ccall((:ibh_turb_k_epsilon, lib), Cint,
        (Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        length(k), k.ptr, ϵ.ptr, S.ptr, par, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, o[5].ptr))
    (νk = o[1], νϵ = o[2], Sk = o[3], Sϵ = o[4], νₜ = o[5])
end
function Turbulence.Wray_Agarwal(R::HipArray{Float32, 1}, S::HipArray{Float32, 1}, ∇R::HipArray{Float32, 2},
                                 ∇S::HipArray{Float32, 2}; σR::Real = 0.72f0, C₁::Real = 0.0829f0, κ::Real = 0.41f0)   # :222-241
    o = ntuple(_ -> _vec_like(R), 3)
    check(ccall((:ibh_turb_wray_agarwal, lib), Cint,
        (Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Cfloat, Cfloat, Cfloat, Ptr{Cvoid},
         Ptr{Cvoid}, Ptr{Cvoid}),
        size(∇R, 2), length(R), R.ptr, S.ptr, ∇R.ptr, ld(∇R), ∇S.ptr, ld(∇S), Float32(σR), Float32(C₁), Float32(κ),
        o[1].ptr, o[2].ptr, o[3].ptr))
    (νₜ = o[1], νR = o[2], S = o[3])
end
function Turbulence.Ducros_sensor(velocity_gradient::AbstractMatrix{<:HipArray})                    # :253-282
    nd, tab = _grad_table(velocity_gradient)
    out = _vec_like(velocity_gradient[1, 1])
    GC.@preserve tab velocity_gradient check(ccall((:ibh_turb_ducros, lib), Cint,
        (Cint, Int64, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}), nd, length(out), tab, out.ptr))
    out
end
function Turbulence.WALE_νSGS(Δ::HipArray{Float32, 1}, velocity_gradient::AbstractMatrix{<:HipArray}; Cw::Real = 0.325f0)   # :292-337
    nd, tab = _grad_table(velocity_gradient)
    @assert nd == 3 "WALE model only implemented for 3D"
    out = _vec_like(Δ)
    GC.@preserve tab velocity_gradient check(ccall((:ibh_turb_wale, lib), Cint,
        (Int64, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cfloat, Ptr{Cvoid}), length(Δ), Δ.ptr, tab, Float32(Cw), out.ptr))
    out
end

# ---------------------------------------------------------------------------------------------------
# CFD.TimeAverage (cfd.jl:738-802): `push!` as ONE launch that updates μ and σ in place (ibh_time_average_push), and
# CFD.pressure_coefficient (cfd.jl:411-424) with M∞^2 folded on the host, as the Python mirror does.
# ---------------------------------------------------------------------------------------------------
const TA_DT_HOST, TA_DT_DEVICE, TA_DT_PER_VAR, TA_DT_ELEMENT = Cint.(0:3)
const TA_F64, TA_FIRST = Cint(1), Cint(2)
function _ta_push(avg::CFD.TimeAverage, Q::HipArray{Float32}, form::Cint, dt::Ptr{Cvoid}, numel::Int, ldd::Int,
                  η::Float64, τ::Float64, flags::Cint)
    check(ccall((:ibh_time_average_push, lib), Cint,
        (Int64, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Cdouble, Cdouble, Cint),
        size(Q, 1), nv(Q), Q.ptr, ld(Q), avg.μ.ptr, avg.σ.ptr, form, dt, numel, ldd, η, τ, flags))
end
"`push!(avg, Q, dt)` (cfd.jl:775-800): η = dt / τ in Julia's promotion of `typeof(avg.τ)` and `typeof(dt)` (Float64 or
Float32; σ^2 and (μ - Q)^2 stay Float32).  `dt` a host scalar, or a device array of one element (no host sync), of
`size(Q, 2)` elements (per variable: the reference's reshape) or of `size(Q)`."
function Base.push!(avg::CFD.TimeAverage, Q::HipArray{Float32}, dt::Union{Real, HipArray{Float32}} = 1.0f0)
    if isnothing(avg.μ)                                       # first registry: μ = copy(Q); σ = μ .* 0
        avg.μ, avg.σ = _vec_like(Q), _vec_like(Q)
        _ta_push(avg, Q, TA_DT_HOST, C_NULL, 0, 0, 0.0, 1.0, TA_FIRST)
        return avg.μ
    end
    size(avg.μ) == size(Q) || throw(DimensionMismatch("push!: Q of size $(size(Q)) after $(size(avg.μ))"))
    if dt isa Real
        η = dt / avg.τ
        f64 = η isa Float64
        _ta_push(avg, Q, TA_DT_HOST, C_NULL, 0, 0, Float64(f64 ? η : Float32(η)),
                 Float64(f64 ? Float64(avg.τ) : Float32(avg.τ)), f64 ? TA_F64 : Cint(0))
    else
        f64 = (1.0f0 / avg.τ) isa Float64
        form, numel, ldd = if length(dt) == 1 && ndims(dt) <= ndims(Q)
            TA_DT_DEVICE, 1, 1
        elseif ndims(Q) == 2 && ndims(dt) == 1 && length(dt) == size(Q, 2)
            TA_DT_PER_VAR, length(dt), length(dt)
        elseif size(dt) == size(Q)
            TA_DT_ELEMENT, length(dt), Int(ld(dt))
        else
            throw(DimensionMismatch("push!: dt of size $(size(dt)) does not broadcast with Q of size $(size(Q))"))
        end
        _ta_push(avg, Q, form, dt.ptr, numel, ldd, 0.0, Float64(f64 ? Float64(avg.τ) : Float32(avg.τ)),
                 f64 ? TA_F64 : Cint(0))
    end
    avg.μ
end
"`pressure_coefficient(fluid, p, p∞, M∞)`: `2 * (p / p∞ - 1) / (M∞^2 * γ)` with `M∞^2 * γ` folded in Float32; the result
is Float32 (the reference's is Float64 for Float64 scalars)."
function CFD.pressure_coefficient(fluid::CFD.Fluid, p::HipArray{Float32}, p∞::Real, M∞::Real)
    M = Float32(M∞)
    s = (M * M) * Float32(fluid.γ)
    pinf = Float32(p∞)
    @. 2 * (p / pinf - 1.0f0) / s
end

# ---------------------------------------------------------------------------------------------------
# Solver.FAS! (src/solver.jl:39-91) on device arrays: the reference's loop with its array passes as library calls --
# `r .+= source; Q .+= clamp(ω, 0, 1) .* r; norm(r)` is ONE launch (ibh_fas_update), the prolongation step another
# (accumulate_diff_add!).  Same keyword arguments, same quirks (recursion guard `length(coarseners) > 1`), same return value.
# ---------------------------------------------------------------------------------------------------
const _norm2 = Ref{Ptr{Cvoid}}(C_NULL)
function _dscalar()
    if _norm2[] == C_NULL
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:ibh_malloc, lib), Cint, (Ptr{Ptr{Cvoid}}, Csize_t), p, 8))
        _norm2[] = p[]
    end
    _norm2[]
end
"`rr = r [.+ source]; [Q .+= clamp(ω, 0, 1) .* rr]`; returns `norm(rr)`."
function _fas_pass(r::HipArray{Float32}, source, Q, ω::Real)
    d = _dscalar()
    check(ccall((:ibh_fas_update, lib), Cint, (Int64, Cfloat, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        length(r), Float32(ω), r.ptr, isnothing(source) ? C_NULL : source.ptr, isnothing(Q) ? C_NULL : Q.ptr, d))
    h = Ref{Float64}(0.0)
    check(ccall((:ibh_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), h, d, 8))
    Float32(sqrt(h[]))
end
function Solver.FAS!(f, Q::HipArray{Float32};
                     coarseners = [], prolongators = [],
                     perscribed_f::Union{HipArray, Nothing} = nothing,
                     multigrid_level::Int = 0, n_iter::Int = 50, rtol::Real = 1.0f-1, atol::Real = 1.0f-7)
    l = multigrid_level
    fQ, ω = f(l, Q)
    source = isnothing(perscribed_f) ? nothing : perscribed_f .- fQ
    nr0 = _fas_pass(fQ, source, nothing, 0f0)
    nr = nr0
    if length(coarseners) > 1
        coars, prolong = to_backend(coarseners[1], hip), to_backend(prolongators[1], hip)
        Qc = coars(Q)
        Qcold = copy(Qc)
        pfQc = coars(isnothing(source) ? fQ : fQ .+ source)
        Solver.FAS!(f, Qc; coarseners = coarseners[2:end], prolongators = prolongators[2:end], perscribed_f = pfQc,
                    multigrid_level = l + 1, n_iter = n_iter, atol = atol, rtol = rtol)
        accumulate_diff_add!(Q, prolong, Qc, Qcold)                  # Q .+= prolongators[1](Qc .- Qcold)
    end
    for _ = 1:n_iter
        r, ω = f(l, Q)
        nr = _fas_pass(r, source, Q, ω)                              # r .+= source; Q .+= clamp(ω, 0, 1) .* r; norm(r)
        nr < nr0 * rtol + atol && break
    end
    nr / (nr0 + eps(Float32))
end
to_backend(a::HipAccumulator, ::Union{typeof(hip), HipConv}) = a

import LinearAlgebra
"`norm(a)` of a device array (what `FAS!` calls, src/solver.jl:57,84): sum of squares in Float64 on the device."
function LinearAlgebra.norm(a::HipArray{Float32})
    d = _dscalar()
    check(ccall((:ibh_sumsq, lib), Cint, (Int64, Ptr{Cvoid}, Ptr{Cvoid}), length(a), a.ptr, d))
    h = Ref{Float64}(0.0)
    check(ccall((:ibh_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), h, d, 8))
    Float32(sqrt(h[]))
end

end # module

# HIPBackend.jl — the reference-side binding a PartitionedArrays.jl (0.2.9)
# maintainer would add (INTEGRATION.md §2).  It plugs libpa_hip.so in behind
# the AbstractBackend / AbstractPData plugin API (src/Interfaces.jl:12, 50):
#
#   * `HIPBackend <: AbstractBackend`, `HIPData{T,N} <: AbstractPData{T,N}`:
#     SequentialBackend semantics (all parts in this process, i_am_main,
#     MAIN = 1) with part p on device devices[mod1(p, end)];
#   * a host/device mirror per part of every PVector and PSparseMatrix
#     (SURVEY.md §7 (i)): host arrays stay the parts the reference's generic
#     code sees; `map_parts` downloads the parts whose device copy is newer
#     before it runs a task and marks them host-newer after; the hot
#     operations upload host-newer parts, run on the device, and mark their
#     outputs device-newer — so a CG loop never touches host memory;
#   * specialisations of the hot path for PVector/PSparseMatrix over HIPData:
#     mul! (Interfaces.jl:2246), exchange!/assemble! of vectors (2071-2106)
#     and matrices (2375-2404), dot/norm/sum (1767, 1973-1992), copyto!/
#     copy!/fill!/rmul! (1649-1680, 1966), broadcasts (1688-1765: the CG
#     patterns by name, any other tree of + - * / abs abs2 conj and
#     comparisons as one pa_vec_eval pass), ==, maximum / minimum, sum of a
#     broadcast, the Euclidean distances (1682-1686, 1774-1863),
#     IterativeSolvers.cg! (v0.9, test_fdm.jl:115), and the COO triplet
#     exchanges assemble!(I, J, V, rows) (2406-2492) and
#     exchange!(I, J, V, rows) (2494-2592), the COO constructor
#     PVector(init, I, V, rows; ids) (1887-1932) and batched reads and writes
#     through global / local ids (view_add!, view_set!, view_get: the
#     global_view / local_view access of 1994-2069 without a download; the
#     same three over the stored entries (i, j) of a PSparseMatrix,
#     2277-2298: the re-assembly loop of a fixed pattern);
#   * everything else (PRange, Exchanger, add_gids!, gather/scatter setup
#     collectives) runs unchanged on the host parts.
#
# Not executed in this repository (no Julia on the build image); the Python
# host package partitionedarrays.jl_amd/ drives the same C-ABI with ctypes and
# is what the tests run.  tests/test_julia_shim.py checks this file
# statically: every helper it calls is defined here, and every ccall names an
# entry point of include/pa_hip.h with its number of arguments.

module HIPBackends

using PartitionedArrays
using LinearAlgebra
using SparseArrays
using SparseMatricesCSR
import IterativeSolvers
import Distances
import PartitionedArrays: get_part_ids, map_parts, i_am_main, get_backend, get_part, gather!,
  gather_all!, scatter, async_exchange!, async_assemble!, num_parts, prun_debug, PVector,
  PSparseMatrix, PRange, SequentialData, AbstractPData, AbstractBackend, Table, Exchanger, MAIN,
  num_lids, num_oids, num_hids, oids_are_equal, hids_are_equal, lids_are_equal

export HIPBackend, HIPData

const libpa = get(ENV, "PA_HIP_LIB", "libpa_hip.so")

# ---- errors (SURVEY.md §8b: int status + pa_last_error) --------------------
function check(rc::Cint)
  rc == 0 && return nothing
  msg = unsafe_string(ccall((:pa_last_error, libpa), Cstring, ()))
  error("libpa_hip: " * msg)
end

const PA_F32, PA_F64, PA_C64, PA_C128 = Cint(0), Cint(1), Cint(2), Cint(3)
dtype_code(::Type{Float32}) = PA_F32
dtype_code(::Type{Float64}) = PA_F64
dtype_code(::Type{ComplexF32}) = PA_C64
dtype_code(::Type{ComplexF64}) = PA_C128
const DeviceEltype = Union{Float32,Float64,ComplexF32,ComplexF64}

function device_count()
  n = Ref{Cint}(0)
  check(ccall((:pa_device_count, libpa), Cint, (Ref{Cint},), n))
  Int(n[])
end

# ---- backend, part contexts ------------------------------------------------
mutable struct PartCtx
  h::Ptr{Cvoid}
  device::Int
  part::Int
end

"""
    HIPBackend(devices=0:ndev-1; share_streams=true)

All parts in this process; part p on device devices[mod1(p, end)].  Parts
on one device share a stream pair (pa_ctx_create_shared) and run each mul!
phase as one grouped launch.  Contexts are created once per partition shape
and reused by every get_part_ids call (get_part_ids(a::AbstractPData) is
called by the generic code, e.g. PRange(parts, n)).
"""
mutable struct HIPBackend <: AbstractBackend
  devices::Vector{Int}
  share_streams::Bool
  ctxs::Dict{Any,Array{PartCtx}}
end
HIPBackend(devices=collect(0:(device_count() - 1)); share_streams::Bool=true) =
  HIPBackend(collect(Int, devices), share_streams, Dict{Any,Array{PartCtx}}())

function _contexts(b::HIPBackend, shape)
  get!(b.ctxs, shape) do
    np = prod(shape)
    isempty(b.devices) && error("HIPBackend: no HIP device visible")
    leader = Dict{Int,PartCtx}()
    cs = map(1:np) do p
      d = b.devices[mod1(p, length(b.devices))]
      h = Ref{Ptr{Cvoid}}(C_NULL)
      if b.share_streams && haskey(leader, d)
        check(ccall((:pa_ctx_create_shared, libpa), Cint, (Cint, Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                    p, np, leader[d].h, h))
      else
        check(ccall((:pa_ctx_create, libpa), Cint, (Cint, Cint, Cint, Ref{Ptr{Cvoid}}), d, p, np, h))
      end
      c = PartCtx(h[], d, p)
      haskey(leader, d) || (leader[d] = c)
      c
    end
    reshape(cs, shape)
  end
end

"""
    HIPData{T,N} <: AbstractPData{T,N}

The parts (host objects: part ids, index sets, host Vectors of PVector
values, SparseMatrixCSC of PSparseMatrix values, ...) plus the part contexts
of the backend.  Device copies hang off the host objects (mirror tables
below), so the parts are exactly what the reference's generic code expects.
"""
struct HIPData{T,N} <: AbstractPData{T,N}
  parts::Array{T,N}
  ctxs::Array{PartCtx,N}
  backend::HIPBackend
end

get_part_ids(b::HIPBackend, nparts::Integer) =
  HIPData(collect(1:nparts), _contexts(b, (nparts,)), b)
get_part_ids(b::HIPBackend, nparts::Tuple) =
  HIPData(collect(LinearIndices(nparts)), _contexts(b, nparts), b)
prun_debug(driver::Function, b::HIPBackend, nparts) = PartitionedArrays.prun(driver, b, nparts)

Base.size(a::HIPData) = size(a.parts)
get_backend(a::HIPData) = a.backend      # the stored backend: no device query, no new contexts
i_am_main(::HIPData) = true
get_part(a::HIPData, part::Integer) = a.parts[part]
get_part(a::HIPData) = get_part(a, MAIN)

# Base.iterate: as SequentialData (SequentialBackend.jl:26-50), so that
# `I, J, V = map_parts(...)` destructures
function Base.iterate(a::HIPData)
  next = map(iterate, a.parts)
  any(isnothing, next) && return nothing
  HIPData(map(first, next), a.ctxs, a.backend), HIPData(map(_second, next), a.ctxs, a.backend)
end
function Base.iterate(a::HIPData, state::HIPData)
  next = map(iterate, a.parts, state.parts)
  any(isnothing, next) && return nothing
  HIPData(map(first, next), a.ctxs, a.backend), HIPData(map(_second, next), a.ctxs, a.backend)
end
_second(a) = a[2]

# map_parts with host/device coherence: the parts of the arguments whose
# device copy is newer are downloaded first; after the task every mirrored
# part of the arguments is taken as modified on the host (the task may write
# any of them; the next hot operation uploads it again).
function map_parts(task, args::HIPData...)
  @assert length(args) > 0
  @assert all(a -> length(a.parts) == length(first(args).parts), args)
  for a in args
    foreach(sync_host!, a.parts)
  end
  parts_out = map(task, map(a -> a.parts, args)...)
  for a in args
    foreach(mark_host_newer!, a.parts)
  end
  HIPData(parts_out, first(args).ctxs, first(args).backend)
end

# host collectives of the setup phase (ids, ptrs, Tables): SequentialBackend's
# (SequentialBackend.jl:73-200) on the host parts
_seq(a::HIPData) = SequentialData(a.parts)
gather!(rcv::HIPData, snd::HIPData) = (gather!(_seq(rcv), _seq(snd)); rcv)
gather_all!(rcv::HIPData, snd::HIPData) = (gather_all!(_seq(rcv), _seq(snd)); rcv)
function scatter(snd::HIPData)
  s = scatter(_seq(snd))
  HIPData(s.parts, snd.ctxs, snd.backend)
end
function async_exchange!(data_rcv::HIPData, data_snd::HIPData, parts_rcv::HIPData,
                         parts_snd::HIPData, t_in::HIPData)
  t = async_exchange!(_seq(data_rcv), _seq(data_snd), _seq(parts_rcv), _seq(parts_snd), _seq(t_in))
  HIPData(t.parts, data_rcv.ctxs, data_rcv.backend)
end

# ---- device mirrors and handle caches ------------------------------------
# state: :host (host copy newer), :device (device copy newer), :both (equal)
mutable struct VecMirror
  h::Ptr{Cvoid}
  state::Symbol
end
mutable struct MatMirror
  h::Ptr{Cvoid}
  nnz::Int
  state::Symbol
end
function _free_vec(m::VecMirror)
  m.h == C_NULL || ccall((:pa_vec_destroy, libpa), Cint, (Ptr{Cvoid},), m.h)
  m.h = C_NULL
end
function _free_mat(m::MatMirror)
  m.h == C_NULL || ccall((:pa_mat_destroy, libpa), Cint, (Ptr{Cvoid},), m.h)
  m.h = C_NULL
end

# Mirror tables keyed by object identity (a content hash of a 16.7 M-value
# part per lookup would cost more than the SpMV): objectid(x) → (WeakRef(x),
# mirror).  An entry whose host object has been collected is stale: the next
# insertion sweeps stale entries and frees their device copies.
const VEC_MIRRORS = Dict{UInt,Tuple{WeakRef,VecMirror}}()  # host part Vector → its pa_vec
const MAT_MIRRORS = Dict{UInt,Tuple{WeakRef,MatMirror}}()  # host part SparseMatrixCSC → its pa_mat
const IDX_CACHE = IdDict{Any,Ptr{Cvoid}}()          # (index set, part, nlids) → pa_index
const XCHG_CACHE = IdDict{Any,Ptr{Cvoid}}()         # (exchanger, part) → pa_xchg
const GIDS_SET = Dict{Ptr{Cvoid},Bool}()          # pa_index handles with their gid table attached
const MXCHG_CACHE = IdDict{Any,Vector{Ptr{Cvoid}}}()  # (matrix exchanger, matrix values) → nz pa_xchg per part

function _mirror(tab, x)
  e = get(tab, objectid(x), nothing)
  (e === nothing || e[1].value !== x) ? nothing : e[2]
end
function _set_mirror!(tab, x, m, free)
  for (k, (w, old)) in collect(tab)   # sweep: host objects gone since the last insertion
    if w.value === nothing
      free(old)
      delete!(tab, k)
    end
  end
  e = get(tab, objectid(x), nothing)
  e === nothing || free(e[2])          # a stale entry under a reused id
  tab[objectid(x)] = (WeakRef(x), m)
  m
end

# download / mark: Vectors through their mirror, views through their parent,
# matrices through theirs; anything else has no device copy
sync_host!(x) = nothing
mark_host_newer!(x) = nothing
function sync_host!(x::Vector)
  m = _mirror(VEC_MIRRORS, x)
  if m !== nothing && m.state === :device
    check(ccall((:pa_vec_download, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), m.h, x, length(x)))
    m.state = :both
  end
  nothing
end
function mark_host_newer!(x::Vector)
  m = _mirror(VEC_MIRRORS, x)
  m === nothing || (m.state = :host)
  nothing
end
sync_host!(x::SubArray) = sync_host!(parent(x))
mark_host_newer!(x::SubArray) = mark_host_newer!(parent(x))
function sync_host!(A::SparseMatrixCSC)
  m = _mirror(MAT_MIRRORS, A)
  if m !== nothing && m.state === :device
    check(ccall((:pa_mat_get_values, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), m.h, nonzeros(A)))
    m.state = :both
  end
  nothing
end
function mark_host_newer!(A::SparseMatrixCSC)
  m = _mirror(MAT_MIRRORS, A)
  m === nothing || (m.state = :host)
  nothing
end
function sync_host!(A::SparseMatrixCSR)
  m = _mirror(MAT_MIRRORS, A)
  if m !== nothing && m.state === :device
    check(ccall((:pa_mat_get_values, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), m.h, nonzeros(A)))
    m.state = :both
  end
  nothing
end
function mark_host_newer!(A::SparseMatrixCSR)
  m = _mirror(MAT_MIRRORS, A)
  m === nothing || (m.state = :host)
  nothing
end
sync_host!(A::PartitionedArrays.SubSparseMatrix) = sync_host!(A.parent)
mark_host_newer!(A::PartitionedArrays.SubSparseMatrix) = mark_host_newer!(A.parent)

function _vec_handle(ctx::PartCtx, x::Vector{T}) where {T<:DeviceEltype}
  m = _mirror(VEC_MIRRORS, x)
  if m === nothing
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_vec_create, libpa), Cint, (Ptr{Cvoid}, Cint, Int64, Ref{Ptr{Cvoid}}),
                ctx.h, dtype_code(T), length(x), out))
    m = _set_mirror!(VEC_MIRRORS, x, VecMirror(out[], :host), _free_vec)
  end
  if m.state === :host
    check(ccall((:pa_vec_upload, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), m.h, x, length(x)))
    m.state = :both
  end
  m.h
end

"""pa_vec handles of the parts of `v` (uploading host-newer parts)."""
dev_vec(v::PVector) = [_vec_handle(v.values.ctxs[i], v.values.parts[i]) for i in eachindex(v.values.parts)]

"""after a device operation wrote `v`: its device copy is the newer one."""
function mark_device_newer!(v::PVector)
  for x in v.values.parts
    m = _mirror(VEC_MIRRORS, x)
    m === nothing || (m.state = :device)
  end
  v
end

function _idx_handle(ctx::PartCtx, ids)
  key = (ids, ctx.part, num_lids(ids))  # add_gid! grows an index set: a new num_lids is a new handle
  get!(IDX_CACHE, key) do
    o = Int32.(collect(ids.oid_to_lid))
    h = Int32.(collect(ids.hid_to_lid))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_index_create, libpa), Cint,
                (Ptr{Cvoid}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Int32}, Ref{Ptr{Cvoid}}),
                ctx.h, num_lids(ids), length(o), o, length(h), h, out))
    out[]
  end
end

"""pa_index handles of the index sets of `r` (IndexSets.jl:215-421)."""
dev_idx(r::PRange) = [_idx_handle(r.partition.ctxs[i], r.partition.parts[i]) for i in eachindex(r.partition.parts)]

function _xchg_handle(ctx::PartCtx, ex::Exchanger, i::Integer)
  get!(XCHG_CACHE, (ex, i)) do
    pr = Int32.(ex.parts_rcv.parts[i]); ps = Int32.(ex.parts_snd.parts[i])
    lr = ex.lids_rcv.parts[i]; ls = ex.lids_snd.parts[i]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_xchg_create, libpa), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32},
                 Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ref{Ptr{Cvoid}}),
                ctx.h, length(pr), pr, Int32.(lr.ptrs), Int32.(lr.data),
                length(ps), ps, Int32.(ls.ptrs), Int32.(ls.data), out))
    out[]
  end
end

"""pa_xchg handles of the Exchanger of `r` (Interfaces.jl:698-713, verbatim)."""
dev_xchg(r::PRange) = [_xchg_handle(r.partition.ctxs[i], r.exchanger, i) for i in eachindex(r.partition.parts)]

function _mat_handle(ctx::PartCtx, A::SparseMatrixCSC{Tv}, rows_h::Ptr{Cvoid}, cols_h::Ptr{Cvoid}) where {Tv<:DeviceEltype}
  m = _mirror(MAT_MIRRORS, A)
  if m !== nothing && m.nnz != nnz(A)  # new pattern: rebuild
    _free_mat(m)
    m = nothing
  end
  if m === nothing
    colptr = Vector{Int64}(A.colptr); rowval = Vector{Int64}(A.rowval)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_mat_from_csc, libpa), Cint,
                (Ptr{Cvoid}, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                ctx.h, dtype_code(Tv), 8, size(A, 1), size(A, 2), colptr, rowval, nonzeros(A),
                rows_h, cols_h, out))
    m = _set_mirror!(MAT_MIRRORS, A, MatMirror(out[], nnz(A), :both), _free_mat)
  elseif m.state === :host  # same pattern, new values (fillstored!, re-assembly)
    check(ccall((:pa_mat_set_values, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), m.h, nonzeros(A)))
    m.state = :both
  end
  m.h
end

# a SparseMatrixCSR{Bi} part (SparseUtils.jl:189-300): pa_mat_from_csr keeps
# the CSR's per-row order and scales each product by α, (v*x)*α (:247)
function _mat_handle(ctx::PartCtx, A::SparseMatrixCSR{Bi,Tv}, rows_h::Ptr{Cvoid}, cols_h::Ptr{Cvoid}) where {Bi,Tv<:DeviceEltype}
  m = _mirror(MAT_MIRRORS, A)
  if m !== nothing && m.nnz != nnz(A)  # new pattern: rebuild
    _free_mat(m)
    m = nothing
  end
  if m === nothing
    rowptr = Vector{Int64}(A.rowptr); colval = Vector{Int64}(A.colval)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_mat_from_csr, libpa), Cint,
                (Ptr{Cvoid}, Cint, Cint, Cint, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                ctx.h, dtype_code(Tv), 8, Bi, size(A, 1), size(A, 2), rowptr, colval, nonzeros(A),
                rows_h, cols_h, out))
    m = _set_mirror!(MAT_MIRRORS, A, MatMirror(out[], nnz(A), :both), _free_mat)
  elseif m.state === :host
    check(ccall((:pa_mat_set_values, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), m.h, nonzeros(A)))
    m.state = :both
  end
  m.h
end

"""pa_mat handles of the parts of `a` (owned-row SELL, built once from the
local SparseMatrixCSC or SparseMatrixCSR; values re-uploaded when the host
copy is newer)."""
function dev_mat(a::PSparseMatrix)
  rh, ch = dev_idx(a.rows), dev_idx(a.cols)
  [_mat_handle(a.values.ctxs[i], a.values.parts[i], rh[i], ch[i]) for i in eachindex(a.values.parts)]
end

function mark_device_newer!(a::PSparseMatrix)
  for A in a.values.parts
    m = _mirror(MAT_MIRRORS, A)
    m === nothing || (m.state = :device)
  end
  a
end

"""pa_xchg handles of the matrix exchanger of `a` (Interfaces.jl:2300-2372;
lids are CSC nz ids, Int64 as Table{Int})."""
function dev_mat_xchg(a::PSparseMatrix)
  A = dev_mat(a)
  get!(MXCHG_CACHE, (a.exchanger, a.values)) do
    ex = a.exchanger
    map(eachindex(a.values.parts)) do i
      pr = Int32.(ex.parts_rcv.parts[i]); ps = Int32.(ex.parts_snd.parts[i])
      lr = ex.lids_rcv.parts[i]; ls = ex.lids_snd.parts[i]
      out = Ref{Ptr{Cvoid}}(C_NULL)
      check(ccall((:pa_mat_xchg_create, libpa), Cint,
                  (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64},
                   Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ref{Ptr{Cvoid}}),
                  A[i], length(pr), pr, Int32.(lr.ptrs), Int64.(lr.data),
                  length(ps), ps, Int32.(ls.ptrs), Int64.(ls.data), out))
      out[]
    end
  end
end

const HIPVector{T} = PVector{T,<:HIPData}
const HIPMatrix{T} = PSparseMatrix{T,<:HIPData}

# ---- completion handles (pa_event) ------------------------------------------
# async_exchange! / async_assemble! on vectors and matrices return one
# unscheduled task per part that waits on that call's own event
# (pa_event_wait): the exchange ran on the part's comm stream and nothing else
# is waited for.  The holder frees the event when it is collected
# (pa_event_destroy is legal while the work is pending).
mutable struct EventHolder
  h::Ptr{Cvoid}
  function EventHolder(h::Ptr{Cvoid})
    e = new(h)
    finalizer(e) do x
      x.h == C_NULL || ccall((:pa_event_destroy, libpa), Cint, (Ptr{Cvoid},), x.h)
      x.h = C_NULL
    end
    e
  end
end
# the tasks this binding created → their events: such a task coming back as
# t0 (Interfaces.jl:369-373) goes to the library as `after`, a device-side
# wait; its closure keeps the holder alive as long as the task lives
const TASK_EVENTS = WeakKeyDict{Task,EventHolder}()

function _event_tasks(done::Vector{Ptr{Cvoid}}, a::HIPData)
  tasks = map(done) do h
    ev = EventHolder(h)
    t = @task check(ccall((:pa_event_wait, libpa), Cint, (Ptr{Cvoid},), ev.h))
    TASK_EVENTS[t] = ev
    t
  end
  HIPData(tasks, a.ctxs, a.backend)
end
# t0 → (the `after` array, the holders to keep alive through the call); a
# task of any other origin is scheduled and waited on the host
function _after(t0::HIPData)
  holders = EventHolder[]
  after = map(t0.parts) do t
    ev = get(TASK_EVENTS, t, nothing)
    if ev === nothing
      istaskstarted(t) || schedule(t)
      wait(t)
      C_NULL
    else
      push!(holders, ev)
      ev.h
    end
  end
  convert(Vector{Ptr{Cvoid}}, after), holders
end
function _after(t0::AbstractPData)
  _wait_all(t0)
  fill(C_NULL, num_parts(t0)), EventHolder[]
end

# the tasks of the COO forms, which size their outputs on the host and have
# completed when they return: waiting on one synchronises its part's streams
function _done_tasks(a::HIPData)
  tasks = map(a.ctxs) do c
    @task check(ccall((:pa_ctx_sync, libpa), Cint, (Ptr{Cvoid},), c.h))
  end
  HIPData(tasks, a.ctxs, a.backend)
end
function _wait_all(t0::AbstractPData)
  map_parts(t0) do t
    istaskstarted(t) || schedule(t)
    wait(t)
  end
  nothing
end

# ---- hot path: mul!(c, a, b, α, β) (Interfaces.jl:2246-2275) --------------
function LinearAlgebra.mul!(c::HIPVector{T}, a::HIPMatrix{T}, b::HIPVector{T}, α::Number, β::Number) where {T<:DeviceEltype}
  @assert oids_are_equal(c.rows, a.rows)
  @assert oids_are_equal(a.cols, b.rows)
  @assert hids_are_equal(a.cols, b.rows)
  A, yv, yi = dev_mat(a), dev_vec(c), dev_idx(c.rows)
  xv, xi, xg = dev_vec(b), dev_idx(b.rows), dev_xchg(b.rows)
  al = Ref{T}(T(α)); be = Ref{T}(T(β))
  check(ccall((:pa_spmv_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
               Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ref{T}, Ref{T}),
              length(A), A, yv, yi, xv, xi, xg, al, be))
  mark_device_newer!(c)
  mark_device_newer!(b)   # exchange!(b): its ghost values were replaced on the device
  c
end
LinearAlgebra.mul!(c::HIPVector{T}, a::HIPMatrix{T}, b::HIPVector{T}) where {T<:DeviceEltype} =
  mul!(c, a, b, one(T), zero(T))
function Base.:*(a::HIPMatrix{Ta}, b::HIPVector{Tb}) where {Ta,Tb}   # Interfaces.jl:2605-2610
  T = typeof(zero(Ta) * zero(Tb) + zero(Ta) * zero(Tb))
  c = PVector{T}(undef, a.rows)
  mul!(c, a, b)
end

# ---- exchange!/assemble! (Interfaces.jl:2071-2106, 2375-2404) --------------
# async_exchange! / async_assemble! call the _async entries: the work runs on
# the parts' comm streams and each returned task waits on its own event, so
# the reference's blocking exchange! / assemble! (schedule + wait over those
# tasks, 453-458) wait for that call alone.  _exchange_all / _mat_exchange_all
# are the library's blocking forms in compute-stream order (no task, nothing
# to wait on before the next call on these parts).
function _exchange_all(v::HIPVector, op::Integer, rev::Integer, zero_ghosts::Integer)
  vv, vi, xg = dev_vec(v), dev_idx(v.rows), dev_xchg(v.rows)
  check(ccall((:pa_exchange_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Cint, Cint),
              length(vv), vv, xg, vi, op, rev, zero_ghosts))
  mark_device_newer!(v)
end
function _exchange_all_async(v::HIPVector, op::Integer, rev::Integer, zero_ghosts::Integer, t0::AbstractPData)
  vv, vi, xg = dev_vec(v), dev_idx(v.rows), dev_xchg(v.rows)
  after, holders = _after(t0)
  done = fill(C_NULL, length(vv))
  GC.@preserve holders check(ccall((:pa_exchange_all_async, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Cint, Cint,
               Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
              length(vv), vv, xg, vi, op, rev, zero_ghosts, after, done))
  mark_device_newer!(v)
  _event_tasks(done, v.values)
end
function async_exchange!(a::HIPVector{T}, t0::AbstractPData=PartitionedArrays._empty_tasks(a.rows.exchanger.parts_rcv)) where {T<:DeviceEltype}
  _exchange_all_async(a, 0, 0, 0, t0)
end
function async_assemble!(a::HIPVector{T}, t0::AbstractPData=PartitionedArrays._empty_tasks(a.rows.exchanger.parts_rcv)) where {T<:DeviceEltype}
  async_assemble!(+, a, t0)
end
function async_assemble!(::typeof(+), a::HIPVector{T}, t0::AbstractPData=PartitionedArrays._empty_tasks(a.rows.exchanger.parts_rcv)) where {T<:DeviceEltype}
  _exchange_all_async(a, 1, 1, 1, t0)   # reverse(exchanger), +, then ghost values = 0
end

function _mat_exchange_all(a::HIPMatrix, op::Integer, rev::Integer, zero_sent::Integer)
  A, mx = dev_mat(a), dev_mat_xchg(a)
  check(ccall((:pa_mat_exchange_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Cint, Cint), length(A), A, mx, op, rev, zero_sent))
  mark_device_newer!(a)
end
function _mat_exchange_all_async(a::HIPMatrix, op::Integer, rev::Integer, zero_sent::Integer, t0::AbstractPData)
  A, mx = dev_mat(a), dev_mat_xchg(a)
  after, holders = _after(t0)
  done = fill(C_NULL, length(A))
  GC.@preserve holders check(ccall((:pa_mat_exchange_all_async, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Cint, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
              length(A), A, mx, op, rev, zero_sent, after, done))
  mark_device_newer!(a)
  _event_tasks(done, a.values)
end
function async_exchange!(a::HIPMatrix{T}, t0::AbstractPData=PartitionedArrays._empty_tasks(a.exchanger.parts_rcv)) where {T<:DeviceEltype}
  _mat_exchange_all_async(a, 0, 0, 0, t0)
end
function async_assemble!(::typeof(+), a::HIPMatrix{T}, t0::AbstractPData=PartitionedArrays._empty_tasks(a.exchanger.parts_rcv)) where {T<:DeviceEltype}
  _mat_exchange_all_async(a, 1, 1, 1, t0)
end
async_assemble!(a::HIPMatrix{T}, t0::AbstractPData=PartitionedArrays._empty_tasks(a.exchanger.parts_rcv)) where {T<:DeviceEltype} =
  async_assemble!(+, a, t0)

# ---- exchange!([combine_op,] values::AbstractPData{<:Table}, exchanger) -----
# (Interfaces.jl:891-961) for HIP parts: rows of any length per lid.  Each
# part's Table gets a pa_table (created once per ptrs Vector: a Table's ptrs
# do not change) whose derived exchanger the library builds on the device and
# keeps; the data goes up before the call and comes back in the part's task.
# Int32 / Int64 data (dof ids) travel as the bits of Float32 / Float64 and can
# only be replaced.
mutable struct TableMirror
  h::Ptr{Cvoid}      # pa_table
  data::Ptr{Cvoid}   # the pa_vec view of its data (owned by the table)
end
function _free_table(m::TableMirror)
  m.h == C_NULL || ccall((:pa_table_destroy, libpa), Cint, (Ptr{Cvoid},), m.h)
  m.h = C_NULL
end
const TABLE_MIRRORS = Dict{UInt,Tuple{WeakRef,TableMirror}}()  # a Table's ptrs Vector → its pa_table
const TableEltype = Union{DeviceEltype,Int32,Int64}
table_carrier(::Type{T}) where {T<:DeviceEltype} = T
table_carrier(::Type{Int32}) = Float32
table_carrier(::Type{Int64}) = Float64

function _table_sizes(m::TableMirror)
  nr = Ref{Int64}(0); nd = Ref{Int64}(0)
  check(ccall((:pa_table_info, libpa), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), m.h, nr, nd))
  Int(nr[]), Int(nd[])
end
"""the ptrs the device holds for a table (1-based), for checks against the host's"""
function _table_ptrs(m::TableMirror)
  p = Vector{Int32}(undef, _table_sizes(m)[1] + 1)
  check(ccall((:pa_table_ptrs, libpa), Cint, (Ptr{Cvoid}, Ptr{Int32}), m.h, p))
  p
end

function _table_handle(ctx::PartCtx, t::Table{T}) where {T<:TableEltype}
  m = _mirror(TABLE_MIRRORS, t.ptrs)
  if m !== nothing && _table_sizes(m) != (length(t.ptrs) - 1, length(t.data))
    m = nothing   # the ptrs Vector was resized in place: a new table (the stale one is freed below)
  end
  if m === nothing
    p32 = convert(Vector{Int32}, t.ptrs)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_table_create, libpa), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}),
                ctx.h, dtype_code(table_carrier(T)), length(p32) - 1, p32, 0, out))
    d = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_table_data, libpa), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), out[], d))
    m = _set_mirror!(TABLE_MIRRORS, t.ptrs, TableMirror(out[], d[]), _free_table)
  end
  check(ccall((:pa_vec_upload, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), m.data, t.data, length(t.data)))
  m
end

_table_op(::typeof(PartitionedArrays._replace), ::Type) = Cint(0)
_table_op(::typeof(+), ::Type{T}) where {T<:DeviceEltype} = Cint(1)
_table_op(::typeof(+), ::Type{T}) where {T<:Integer} =
  error("exchange!(+, Table): integer tables travel as bit patterns and cannot be added on the device")
_table_op(op, ::Type) = error("exchange!(combine_op, Table) on HIP parts: combine_op must be replace or +")

function _table_handles(values::HIPData{<:Table}, exchanger::Exchanger)
  ms = [_table_handle(values.ctxs[i], values.parts[i]) for i in eachindex(values.parts)]
  xg = [_xchg_handle(values.ctxs[i], exchanger, i) for i in eachindex(values.parts)]
  ms, convert(Vector{Ptr{Cvoid}}, [m.h for m in ms]), xg
end
function _table_download(m::TableMirror, t::Table)
  check(ccall((:pa_vec_download, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), m.data, t.data, length(t.data)))
end

# the blocking form in compute-stream order (no task), any (op, reverse, zero_sent)
function _table_exchange_all(values::HIPData{<:Table{T}}, exchanger::Exchanger, op::Integer, rev::Integer,
                             zero_sent::Integer) where {T<:TableEltype}
  ms, tb, xg = _table_handles(values, exchanger)
  check(ccall((:pa_table_exchange_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Cint, Cint), length(tb), tb, xg, op, rev, zero_sent))
  foreach(_table_download, ms, values.parts)
  values
end

function async_exchange!(combine_op, values::HIPData{<:Table{T}}, exchanger::Exchanger,
                         t0::AbstractPData=PartitionedArrays._empty_tasks(exchanger.parts_rcv)) where {T<:TableEltype}
  op = _table_op(combine_op, T)
  ms, tb, xg = _table_handles(values, exchanger)
  after, holders = _after(t0)
  done = fill(C_NULL, length(tb))
  GC.@preserve holders check(ccall((:pa_table_exchange_all_async, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Cint, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
              length(tb), tb, xg, op, 0, 0, after, done))
  # a part's task waits for its event, then brings the data back into the host Table
  tasks = map(eachindex(done)) do i
    ev = EventHolder(done[i])
    m, t = ms[i], values.parts[i]
    task = @task begin
      check(ccall((:pa_event_wait, libpa), Cint, (Ptr{Cvoid},), ev.h))
      _table_download(m, t)
    end
    TASK_EVENTS[task] = ev
    task
  end
  HIPData(tasks, values.ctxs, values.backend)
end

# fillstored!(a, v) (Interfaces.jl:2127-2132) on the device copies; the host
# parts are refreshed on their next generic use (sync_host!)
function LinearAlgebra.fillstored!(a::HIPMatrix{T}, v) where {T<:DeviceEltype}
  A = dev_mat(a)
  s = Ref{T}(convert(T, v))
  for h in A
    check(ccall((:pa_mat_fillstored, libpa), Cint, (Ptr{Cvoid}, Ptr{T}), h, s))
  end
  mark_device_newer!(a)
  a
end

# ---- assemble!(I, J, V, rows) (Interfaces.jl:2406-2492) --------------------
# the triplets go to the device (pa_coo), the ghost rows' triplets move to
# their owners there (pa_coo_assemble_all: device copies / RCCL), and the
# assembled lists come back into I, J, V (resize!, as the reference does)
function _idx_gids_handle(ctx::PartCtx, ids)
  h = _idx_handle(ctx, ids)
  get!(GIDS_SET, h) do
    g = Int64.(collect(ids.lid_to_gid))
    check(ccall((:pa_index_set_gids, libpa), Cint, (Ptr{Cvoid}, Ptr{Int64}), h, g))
    true
  end
  h
end
# to_ghosts = false: pa_coo_assemble_all; true: pa_coo_exchange_all
function _coo_all!(to_ghosts::Bool, I::HIPData, J::HIPData, V::HIPData{<:Vector{T}}, rows::PRange) where {T}
  n = length(I.parts)
  coo = Vector{Ptr{Cvoid}}(undef, n)
  for i in 1:n
    out = Ref{Ptr{Cvoid}}(C_NULL)
    gi = Int64.(I.parts[i]); gj = Int64.(J.parts[i])
    check(ccall((:pa_coo_create, libpa), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{T}, Ref{Ptr{Cvoid}}),
                I.ctxs[i].h, dtype_code(T), length(gi), gi, gj, V.parts[i], out))
    coo[i] = out[]
  end
  try
    ri = [_idx_gids_handle(rows.partition.ctxs[i], rows.partition.parts[i]) for i in 1:n]
    if to_ghosts
      check(ccall((:pa_coo_exchange_all, libpa), Cint,
                  (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}), n, coo, ri, dev_xchg(rows)))
    else
      check(ccall((:pa_coo_assemble_all, libpa), Cint,
                  (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}), n, coo, ri, dev_xchg(rows)))
    end
    for i in 1:n
      m = Ref{Int64}(0)
      check(ccall((:pa_coo_size, libpa), Cint, (Ptr{Cvoid}, Ref{Int64}), coo[i], m))
      gi = Vector{Int64}(undef, m[]); gj = Vector{Int64}(undef, m[])
      resize!(V.parts[i], m[])
      check(ccall((:pa_coo_download, libpa), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{T}),
                  coo[i], gi, gj, V.parts[i]))
      resize!(I.parts[i], m[]); I.parts[i] .= gi
      resize!(J.parts[i], m[]); J.parts[i] .= gj
    end
  finally
    foreach(h -> ccall((:pa_coo_destroy, libpa), Cint, (Ptr{Cvoid},), h), coo)
  end
  _done_tasks(I)
end
function async_assemble!(I::HIPData{<:Vector{<:Integer}}, J::HIPData{<:Vector{<:Integer}},
                         V::HIPData{<:Vector{T}}, rows::PRange,
                         t0::AbstractPData=PartitionedArrays._empty_tasks(rows.exchanger.parts_rcv)) where {T<:DeviceEltype}
  _wait_all(t0)
  _coo_all!(false, I, J, V, rows)
end

# ---- exchange!(I, J, V, rows) (Interfaces.jl:2494-2592) --------------------
# the mirror of the assembly: the owners' triplets of the rows that other
# parts hold as ghosts are copied to those parts on the device
# (pa_coo_exchange_all; a row held by several neighbours goes to the last of
# them in parts_snd order, as the reference's lid_to_i does), unsent ghost
# rows' values become zero(T); exchange! itself is the reference's generic
# schedule-and-wait over the tasks returned here (453-458)
function async_exchange!(I::HIPData{<:Vector{<:Integer}}, J::HIPData{<:Vector{<:Integer}},
                         V::HIPData{<:Vector{T}}, rows::PRange,
                         t0::AbstractPData=PartitionedArrays._empty_tasks(rows.exchanger.parts_rcv)) where {T<:DeviceEltype}
  _wait_all(t0)
  _coo_all!(true, I, J, V, rows)
end

# ---- PVector(init, I, V, rows; ids) and the indexed views -------------------
# The COO constructor (Interfaces.jl:1887-1910) and the batched forms of
# `view[I] .+= V`, `view[I] = V` and `view[I]` over global_view / local_view
# (1994-2069) as one ordered scatter / gather per part (pa_vec_scatter,
# pa_vec_gather): values[lid] += V[i] in input order, bit for bit the
# reference's loop.  PVector(init, I, V, n; ids) (1920-1932) reaches the
# constructor below through the reference's own method (PRange, add_gids!).
const PA_IDS_LOCAL, PA_IDS_GLOBAL = Cint(0), Cint(1)
const PA_SCATTER_ADD, PA_SCATTER_SET = Cint(0), Cint(1)
_ids_kind(ids::Symbol) = ids === :global ? PA_IDS_GLOBAL : PA_IDS_LOCAL
# the ids as the library takes them: Int64 gids, Int32 or Int64 lids (a copy
# unless they already are such a Vector; gids are translated in it)
_ids_vector(I::Vector{Int64}, ids::Symbol) = I
_ids_vector(I::Vector{Int32}, ids::Symbol) = ids === :global ? Int64.(I) : I
_ids_vector(I::AbstractArray{<:Integer}, ids::Symbol) = Int64.(collect(I))

function _vec_scatter!(h::Ptr{Cvoid}, ih::Ptr{Cvoid}, ids::Symbol, op::Cint, zero_first::Bool,
                       I::Vector{Ti}, V::Vector{T}) where {Ti<:Union{Int32,Int64},T<:DeviceEltype}
  @assert length(I) == length(V)
  check(ccall((:pa_vec_scatter, libpa), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Int64, Ptr{Ti}, Ptr{T}),
              h, ih, _ids_kind(ids), Cint(sizeof(Ti)), op, Cint(zero_first), Cint(0), length(I), I, V))
end
function _vec_gather(h::Ptr{Cvoid}, ih::Ptr{Cvoid}, ids::Symbol, absent_zero::Bool,
                     I::Vector{Ti}, ::Type{T}) where {Ti<:Union{Int32,Int64},T<:DeviceEltype}
  out = Vector{T}(undef, length(I))
  check(ccall((:pa_vec_gather, libpa), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Int64, Ptr{Ti}, Ptr{T}),
              h, ih, _ids_kind(ids), Cint(sizeof(Ti)), Cint(absent_zero), Cint(0), length(I), I, out))
  out
end
# the same over device arrays of the caller (a ROCArray's pointer, next to
# pa_vec_device_ptr): on_device = 1, ids of index_bytes bytes each
function _vec_scatter_dev!(h::Ptr{Cvoid}, ih::Ptr{Cvoid}, ids::Symbol, op::Cint, zero_first::Bool,
                           index_bytes::Integer, n::Integer, dI::Ptr{Cvoid}, dV::Ptr{Cvoid})
  check(ccall((:pa_vec_scatter, libpa), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
              h, ih, _ids_kind(ids), Cint(index_bytes), op, Cint(zero_first), Cint(1), n, dI, dV))
end
function _vec_gather_dev!(h::Ptr{Cvoid}, ih::Ptr{Cvoid}, ids::Symbol, absent_zero::Bool,
                          index_bytes::Integer, n::Integer, dI::Ptr{Cvoid}, dout::Ptr{Cvoid})
  check(ccall((:pa_vec_gather, libpa), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
              h, ih, _ids_kind(ids), Cint(index_bytes), Cint(absent_zero), Cint(1), n, dI, dout))
end

_view_idx(a::PVector, ids::Symbol) =
  [(ids === :global ? _idx_gids_handle : _idx_handle)(a.rows.partition.ctxs[i], a.rows.partition.parts[i])
   for i in eachindex(a.rows.partition.parts)]

# op over every part; with ids = :global the Int64 vectors of I hold lids afterwards
function _scatter_parts!(a::HIPVector{T}, hs, I::HIPData, V::HIPData, ids::Symbol, op::Cint,
                         zero_first::Bool, translate::Bool) where {T<:DeviceEltype}
  @assert ids in (:global, :local)
  ih = _view_idx(a, ids)
  for i in eachindex(a.values.parts)
    Ii = _ids_vector(I.parts[i], ids)
    ids === :global && !translate && Ii === I.parts[i] && (Ii = copy(Ii))
    _vec_scatter!(hs[i], ih[i], ids, op, zero_first, Ii, convert(Vector{T}, V.parts[i]))
    ids === :global && translate && Ii !== I.parts[i] && (I.parts[i] .= Ii)
  end
  mark_device_newer!(a)
end

function PVector(init, I::HIPData{<:AbstractArray{<:Integer}}, V::HIPData{<:AbstractArray},
                 rows::PRange; ids::Symbol)
  @assert ids in (:global, :local)
  values = map_parts(partition -> init(num_lids(partition)), rows.partition)
  a = PVector(values, rows)
  if !(eltype(a) <: DeviceEltype)   # e.g. the Int vectors of test_interfaces.jl: the host loop
    ids === :global && PartitionedArrays.to_lids!(I, rows)
    map_parts(values, I, V) do values, I, V
      fill!(values, zero(eltype(values)))
      for i in 1:length(I)
        values[I[i]] += V[i]
      end
    end
    return a
  end
  # fill!(values, zero(T)) and the loop on the device; I is translated in
  # place for ids = :global, as to_lids! does in the reference (1895-1897)
  _scatter_parts!(a, dev_vec_nocopy(a), I, V, ids, PA_SCATTER_ADD, true, true)
end

"""`view[I[k]] += V[k]` for every k in input order, over `global_view(a, a.rows)`
(ids = :global) or `local_view(a, a.rows)` (ids = :local), per part, on the device."""
view_add!(a::HIPVector, I::HIPData, V::HIPData; ids::Symbol) =
  _scatter_parts!(a, dev_vec(a), I, V, ids, PA_SCATTER_ADD, false, false)
"""`view[I[k]] = V[k]` in input order (a repeated id keeps its last value)."""
view_set!(a::HIPVector, I::HIPData, V::HIPData; ids::Symbol) =
  _scatter_parts!(a, dev_vec(a), I, V, ids, PA_SCATTER_SET, false, false)
"""`view[I]` per part.  A gid that is not a local id reads zero(T) with
absent_zero (LocalView, Interfaces.jl:2019-2026) and is an error without
(GlobalView, 2062-2065)."""
function view_get(a::HIPVector{T}, I::HIPData; ids::Symbol, absent_zero::Bool=false) where {T<:DeviceEltype}
  @assert ids in (:global, :local)
  hs, ih = dev_vec(a), _view_idx(a, ids)
  out = [_vec_gather(hs[i], ih[i], ids, absent_zero, _ids_vector(I.parts[i], ids), T)
         for i in eachindex(a.values.parts)]
  HIPData(out, a.values.ctxs, a.values.backend)
end

# ---- entry views of a PSparseMatrix (Interfaces.jl:2277-2298) ---------------
# The batched forms of `view[i, j] += v`, `view[i, j] = v` and `view[i, j]`
# over global_view(a, a.rows, a.cols) (ids = :global) / local_view(a, a.rows,
# a.cols) (ids = :local), one pa_mat_scatter / pa_mat_gather per part over the
# stored entries: the re-assembly loop of a fixed pattern without a download
# of nzval.  I and J are left as they are; an (i, j) the pattern does not
# store reads zero(T) and cannot be written (the device pattern is fixed).
function _mat_scatter!(h::Ptr{Cvoid}, rh::Ptr{Cvoid}, ch::Ptr{Cvoid}, ids::Symbol, op::Cint,
                       I::Vector{Ti}, J::Vector{Ti}, V::Vector{T}) where {Ti<:Union{Int32,Int64},T<:DeviceEltype}
  @assert length(I) == length(J) == length(V)
  check(ccall((:pa_mat_scatter, libpa), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Int64, Ptr{Ti}, Ptr{Ti}, Ptr{T}),
              h, rh, ch, _ids_kind(ids), Cint(sizeof(Ti)), op, Cint(0), length(I), I, J, V))
end
function _mat_gather(h::Ptr{Cvoid}, rh::Ptr{Cvoid}, ch::Ptr{Cvoid}, ids::Symbol, absent_zero::Bool,
                     I::Vector{Ti}, J::Vector{Ti}, ::Type{T}) where {Ti<:Union{Int32,Int64},T<:DeviceEltype}
  @assert length(I) == length(J)
  out = Vector{T}(undef, length(I))
  check(ccall((:pa_mat_gather, libpa), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Cint, Int64, Ptr{Ti}, Ptr{Ti}, Ptr{T}),
              h, rh, ch, _ids_kind(ids), Cint(sizeof(Ti)), Cint(absent_zero), Cint(0), length(I), I, J, out))
  out
end
# row and column ids in one width (Int32 only when both are Int32 lids)
function _ids_pair(I, J, ids::Symbol)
  Ii, Ji = _ids_vector(I, ids), _ids_vector(J, ids)
  eltype(Ii) === eltype(Ji) ? (Ii, Ji) : (Int64.(Ii), Int64.(Ji))
end
_mat_view_idx(r::PRange, ids::Symbol) =
  [(ids === :global ? _idx_gids_handle : _idx_handle)(r.partition.ctxs[i], r.partition.parts[i])
   for i in eachindex(r.partition.parts)]

function _mat_scatter_parts!(a::HIPMatrix{T}, I::HIPData, J::HIPData, V::HIPData, ids::Symbol,
                             op::Cint) where {T<:DeviceEltype}
  @assert ids in (:global, :local)
  hs = dev_mat(a)
  rh, ch = _mat_view_idx(a.rows, ids), _mat_view_idx(a.cols, ids)
  for i in eachindex(a.values.parts)
    Ii, Ji = _ids_pair(I.parts[i], J.parts[i], ids)
    _mat_scatter!(hs[i], rh[i], ch[i], ids, op, Ii, Ji, convert(Vector{T}, V.parts[i]))
  end
  mark_device_newer!(a)
end

"""`view[I[k], J[k]] += V[k]` for every k in input order, over
`global_view(a, a.rows, a.cols)` (ids = :global) or `local_view(a, a.rows,
a.cols)` (ids = :local), per part, on the device."""
view_add!(a::HIPMatrix, I::HIPData, J::HIPData, V::HIPData; ids::Symbol) =
  _mat_scatter_parts!(a, I, J, V, ids, PA_SCATTER_ADD)
"""`view[I[k], J[k]] = V[k]` in input order (a repeated (i, j) keeps its last value)."""
view_set!(a::HIPMatrix, I::HIPData, J::HIPData, V::HIPData; ids::Symbol) =
  _mat_scatter_parts!(a, I, J, V, ids, PA_SCATTER_SET)
"""`view[I[k], J[k]]` per part; an entry the pattern does not store reads
zero(T).  A gid that is not a local id reads zero(T) with absent_zero
(LocalView, Interfaces.jl:2019-2026) and is an error without (GlobalView,
2062-2065)."""
function view_get(a::HIPMatrix{T}, I::HIPData, J::HIPData; ids::Symbol, absent_zero::Bool=false) where {T<:DeviceEltype}
  @assert ids in (:global, :local)
  hs = dev_mat(a)
  rh, ch = _mat_view_idx(a.rows, ids), _mat_view_idx(a.cols, ids)
  out = map(eachindex(a.values.parts)) do i
    Ii, Ji = _ids_pair(I.parts[i], J.parts[i], ids)
    _mat_gather(hs[i], rh[i], ch[i], ids, absent_zero, Ii, Ji, T)
  end
  HIPData(out, a.values.ctxs, a.values.backend)
end

# ---- findnz on the device, to_gids! and gather(A) (Interfaces.jl:2664-2704) -
# pa_mat_findnz reads a part's stored entries back in the parent's nziterator
# order (the loop of 2669-2689 with its owned-row filter); gather(A) below is
# the reference's method with that loop replaced, so A \ b, lu, lu! and ldiv!
# (2626-2662) take the matrix from the device without a host copy of nzval.
const PA_NZ_OWNED_ROWS, PA_NZ_ALL_ROWS = Cint(0), Cint(1)

"""(I, J, V) of the stored entries of every part: `rows = :owned` the rows the
part owns, `:all` the stored ghost rows too; `ids = :global` gids, `:local`
lids of a.rows / a.cols."""
function dev_findnz(a::HIPMatrix{T}; rows::Symbol=:owned, ids::Symbol=:global) where {T<:DeviceEltype}
  @assert rows in (:owned, :all) && ids in (:global, :local)
  hs = dev_mat(a)
  rh, ch = _mat_view_idx(a.rows, ids), _mat_view_idx(a.cols, ids)
  out = map(eachindex(a.values.parts)) do i
    coo = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pa_mat_findnz, libpa), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}),
                hs[i], rh[i], ch[i], rows === :all ? PA_NZ_ALL_ROWS : PA_NZ_OWNED_ROWS, _ids_kind(ids), coo))
    try
      m = Ref{Int64}(0)
      check(ccall((:pa_coo_size, libpa), Cint, (Ptr{Cvoid}, Ref{Int64}), coo[], m))
      I = Vector{Int64}(undef, m[]); J = Vector{Int64}(undef, m[]); V = Vector{T}(undef, m[])
      check(ccall((:pa_coo_download, libpa), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{T}),
                  coo[], I, J, V))
      (I, J, V)
    finally
      ccall((:pa_coo_destroy, libpa), Cint, (Ptr{Cvoid},), coo[])
    end
  end
  ntuple(k -> HIPData([o[k] for o in out], a.values.ctxs, a.values.backend), 3)
end

function PartitionedArrays.to_gids!(I::HIPData{<:Vector{Int64}}, a::PRange)
  for i in eachindex(I.parts)
    h = _idx_gids_handle(a.partition.ctxs[i], a.partition.parts[i])
    check(ccall((:pa_index_to_gids, libpa), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}),
                h, length(I.parts[i]), I.parts[i]))
  end
  I
end

function PartitionedArrays.gather(a::HIPMatrix{T},
                                  rows_in_main::PRange=PartitionedArrays._to_main(a.rows),
                                  cols_in_main::PRange=PartitionedArrays._to_main(a.cols)) where {T<:DeviceEltype}
  I, J, V = dev_findnz(a; rows=:owned, ids=:global)
  assemble!(I, J, V, rows_in_main)
  for i in eachindex(I.parts)
    if a.rows.partition.parts[i].part != MAIN
      resize!(I.parts[i], 0); resize!(J.parts[i], 0); resize!(V.parts[i], 0)
    end
  end
  M = eltype(a.values)
  exchanger = PartitionedArrays.empty_exchanger(rows_in_main.partition)
  PSparseMatrix((args...) -> PartitionedArrays.compresscoo(M, args...),
                I, J, V, rows_in_main, cols_in_main, exchanger; ids=:global)
end

# ---- reductions (Interfaces.jl:221-238, 1767-1772, 1973-1992) -------------
function LinearAlgebra.dot(a::HIPVector{T}, b::HIPVector{T}) where {T<:DeviceEltype}
  r = Ref{T}(zero(T))
  check(ccall((:pa_dot_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ref{T}),
              num_parts(a.values), dev_vec(a), dev_idx(a.rows), dev_vec(b), dev_idx(b.rows), r))
  r[]
end
function LinearAlgebra.norm(a::HIPVector{T}, p::Real=2) where {T<:DeviceEltype}
  # p = 1 and p = Inf of real vectors: sum(abs.(a)) and maximum(abs, a) in one pass
  p == 1 && T <: Real && return sum(_expr_node(abs, a))
  p == Inf && T <: Real && return maximum(abs, a)
  p == 2 || return invoke(norm, Tuple{PVector,Real}, a, p)
  r = Ref{Float64}(0.0)
  check(ccall((:pa_norm2_all, libpa), Cint, (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ref{Float64}),
              num_parts(a.values), dev_vec(a), dev_idx(a.rows), r))
  r[]
end
function Base.sum(a::HIPVector{T}) where {T<:DeviceEltype}
  r = Ref{T}(zero(T))
  check(ccall((:pa_sum_all, libpa), Cint, (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ref{T}),
              num_parts(a.values), dev_vec(a), dev_idx(a.rows), r))
  r[]
end

# ---- vector updates (Interfaces.jl:1649-1680, 1688-1765, 1966-1971) -------
function Base.fill!(a::HIPVector{T}, v) where {T<:DeviceEltype}
  s = Ref{T}(T(v))
  for (h, x) in zip(dev_vec_nocopy(a), a.values.parts)
    check(ccall((:pa_vec_fill, libpa), Cint, (Ptr{Cvoid}, Ref{T}), h, s))
  end
  mark_device_newer!(a)
end
# a vector about to be overwritten everywhere: its host values need not be uploaded
function dev_vec_nocopy(v::PVector)
  map(eachindex(v.values.parts)) do i
    x = v.values.parts[i]
    m = _mirror(VEC_MIRRORS, x)
    if m === nothing
      m = _vec_handle_uninit(v.values.ctxs[i], x)
    elseif m.state === :host
      m.state = :both   # about to be overwritten on the device: no upload
    end
    m.h
  end
end
function _vec_handle_uninit(ctx::PartCtx, x::Vector{T}) where {T<:DeviceEltype}
  out = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:pa_vec_create, libpa), Cint, (Ptr{Cvoid}, Cint, Int64, Ref{Ptr{Cvoid}}),
              ctx.h, dtype_code(T), length(x), out))
  _set_mirror!(VEC_MIRRORS, x, VecMirror(out[], :both), _free_vec)
end

function Base.copyto!(a::HIPVector{T}, b::HIPVector{T}) where {T<:DeviceEltype}
  @assert oids_are_equal(a.rows, b.rows)
  same = a.rows.partition === b.rows.partition
  src = dev_vec(b)
  dst = same ? dev_vec_nocopy(a) : dev_vec(a)
  ia, ib = dev_idx(a.rows), dev_idx(b.rows)
  for i in eachindex(dst)
    check(ccall((:pa_vec_copy, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint),
                dst[i], ia[i], src[i], ib[i], same ? 1 : 0))
  end
  mark_device_newer!(a)
end
Base.copy!(a::HIPVector{T}, b::HIPVector{T}) where {T<:DeviceEltype} = copyto!(a, b)

# the scalar as Julia's broadcast types it: a Float64 (Real * Complex
# componentwise) or a ComplexF64 that widens T is passed as such and the
# elements are evaluated in Float64 / ComplexF64 (PA_BCAST_F64 / _C128);
# anything else is converted to T
const PA_BCAST_F64, PA_BCAST_C128 = Cint(8), Cint(16)
_bcast_scalar(::Type{T}, a::Float64) where {T} = (Ref{Float64}(a), PA_BCAST_F64)
_bcast_scalar(::Type{T}, a::ComplexF64) where {T<:Complex} = (Ref{ComplexF64}(a), PA_BCAST_C128)
_bcast_scalar(::Type{T}, a) where {T} = (Ref{T}(T(a)), Cint(0))

# the named pattern `mode` as a tree over y and x; the scalar keeps
# _bcast_scalar's typing (anything but a widening Float64 / ComplexF64 is a T)
function _axpby_tree(y::HIPVector{T}, x::HIPVector{T}, a, mode::Integer) where {T<:DeviceEltype}
  s = (a isa Float64 || (a isa ComplexF64 && T <: Complex)) ? a : T(a)
  mode == 0 && return _expr_node(+, x, _expr_node(*, s, y))
  mode == 1 && return _expr_node(+, y, _expr_node(*, s, x))
  mode == 2 && return _expr_node(-, y, _expr_node(*, s, x))
  _expr_node(-, y, x)
end

function _axpby!(y::HIPVector{T}, x::Union{Nothing,HIPVector{T}}, a, mode::Integer) where {T<:DeviceEltype}
  all_lids = x === nothing || y.rows === x.rows
  x === nothing || all_lids || @assert oids_are_equal(y.rows, x.rows)
  # pa_vec_axpby reads x through y's index set: only for one lid layout.  Equal
  # owned ids in another lid order (or next to other ghosts) go through
  # pa_vec_eval, which carries one index set per operand.
  if x !== nothing && !all_lids && !lids_are_equal(y.rows, x.rows)
    bc = _axpby_tree(y, x, a, mode)
    return _expr_eval!(y, _expr_encode(T, bc), bc)
  end
  s, kind = _bcast_scalar(T, a)
  yv, xv, iy = dev_vec(y), (x === nothing ? fill(C_NULL, num_parts(y.values)) : dev_vec(x)), dev_idx(y.rows)
  for i in eachindex(yv)
    check(ccall((:pa_vec_axpby, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint),
                yv[i], xv[i], iy[i], s, Cint(mode) | kind, all_lids ? 1 : 0))
  end
  mark_device_newer!(y)
end
LinearAlgebra.rmul!(a::HIPVector{T}, v::Number) where {T<:DeviceEltype} = _axpby!(a, nothing, v, 4)

# Broadcasts: a lazy tree over HIP vectors; materialize! runs the patterns of
# the CG recurrence on the device by name (pa_vec_axpby modes 0-3, copies),
# any other tree of the supported functions as one postfix program
# (pa_vec_eval), and only trees with other functions through the reference's
# host broadcast on synced parts.
struct HIPBroadcasted{F,A}
  f::F
  args::A
  rows::PRange
end
const HIPArg = Union{HIPVector,HIPBroadcasted}
_rows(a::HIPVector) = a.rows
_rows(a::HIPBroadcasted) = a.rows
Base.broadcasted(f, args::HIPArg...) = HIPBroadcasted(f, args, _rows(first(args)))
Base.broadcasted(f, a::Number, b::HIPArg) = HIPBroadcasted(f, (a, b), _rows(b))
Base.broadcasted(f, a::HIPArg, b::Number) = HIPBroadcasted(f, (a, b), _rows(a))

_scaled(b) = nothing
function _scaled(b::HIPBroadcasted)   # β .* u or u .* β
  b.f === (*) && length(b.args) == 2 || return nothing
  a1, a2 = b.args
  a1 isa Number && a2 isa HIPVector && return (a1, a2)
  a1 isa HIPVector && a2 isa Number && return (a2, a1)
  nothing
end

# (mode, x, scalar) of y .= expression, or nothing
function _axpby_pattern(y::HIPVector, bc::HIPBroadcasted)
  length(bc.args) == 2 || return (bc.f === identity && length(bc.args) == 1 && bc.args[1] isa HIPVector) ?
                                 (:copy, bc.args[1], nothing) : nothing
  a1, a2 = bc.args
  if bc.f === (+)
    s = _scaled(a2)
    s !== nothing && a1 isa HIPVector && s[2] === y && return (0, a1, s[1])   # u .= r .+ β.*u
    s !== nothing && a1 === y && return (1, s[2], s[1])                         # x .+= α.*u
  elseif bc.f === (-)
    s = _scaled(a2)
    s !== nothing && a1 === y && return (2, s[2], s[1])                         # r .-= α.*c
    a1 === y && a2 isa HIPVector && return (3, a2, nothing)                      # r .-= c
  end
  nothing
end

function Base.materialize!(y::HIPVector{T}, bc::HIPBroadcasted) where {T<:DeviceEltype}
  pat = _axpby_pattern(y, bc)
  # device patterns over vectors of y's partition (all lids, as the
  # reference's materialize! does when every argument shares y.rows)
  if pat !== nothing && (pat[2] isa HIPVector{T}) && pat[2].rows === y.rows
    mode, x, a = pat
    mode === :copy && return copyto!(y, x)
    return _axpby!(y, x, a === nothing ? zero(T) : a, mode)
  end
  # any other tree of the supported functions: one pass on the device
  prog = _expr_encode(T, bc)
  prog === nothing || return _expr_eval!(y, prog, bc)
  # trees with other functions: the reference's host broadcast (Interfaces.jl:1688-1765)
  host = _host_broadcasted(bc)
  invoke(Base.materialize!, Tuple{PVector,PartitionedArrays.DistributedBroadcasted}, y, host)
end
Base.materialize!(y::PVector, bc::HIPBroadcasted) =
  invoke(Base.materialize!, Tuple{PVector,PartitionedArrays.DistributedBroadcasted}, y, _host_broadcasted(bc))
function Base.materialize(bc::HIPBroadcasted)
  T = _expr_eltype(bc)
  prog = T === nothing ? nothing : _expr_encode(T, bc)
  prog === nothing && return Base.materialize(_host_broadcasted(bc))
  _expr_eval!(PVector{T}(undef, bc.rows), prog, bc)   # Interfaces.jl:1694-1708
end

# ---- broadcast expressions as postfix programs (include/pa_hip.h: pa_expr) --
# The tree's functions map to op codes; every node is tagged with its type as
# Julia's broadcast infers it (T, or the wide type when an operand is a
# Float64 / ComplexF64 scalar or a wide node; real valued over complex T for
# a Float64 scalar, abs2 and comparisons).  Of two sibling subtrees the one
# that needs more stack slots is emitted first (the reversed operand mode
# keeps left ∘ right); scalars ride as immediates of their op.  A tree the
# program cannot hold (other functions, too deep, too long, complex division)
# encodes to `nothing` and takes the host path.
const PA_EXPR_MAX_OPS, PA_EXPR_MAX_VECS, PA_EXPR_MAX_SCALARS, PA_EXPR_MAX_DEPTH = 32, 8, 8, 4
const PA_EXPR_WIDE, PA_EXPR_LREAL, PA_EXPR_RREAL = 0x01, 0x02, 0x04
const PA_EXPR_SS, PA_EXPR_SC, PA_EXPR_CS, PA_EXPR_RS = 0x00, 0x08, 0x10, 0x18
const PA_REDUCE_SUM, PA_REDUCE_MAX, PA_REDUCE_MIN = Cint(0), Cint(1), Cint(2)
struct PaExprOp
  code::UInt8
  arg::UInt8
  flags::UInt8
  pad::UInt8
end
struct PaExpr
  nops::Int32
  ops::NTuple{32,PaExprOp}
end
mutable struct ExprEncoder
  vecs::Vector{Any}          # distinct HIPVector operands
  scal::Vector{UInt8}        # 16-byte scalar slots
  kinds::Vector{Cint}        # 0 element type, 1 Float64, 2 ComplexF64, 3 real(T)
  ops::Vector{PaExprOp}
  sp::Int
  depth::Int
end

function _binary_code(f)
  f === (+) && return 2
  f === (-) && return 3
  f === (*) && return 4
  f === (/) && return 5
  f === (<) && return 10
  f === (<=) && return 11
  f === (>) && return 12
  f === (>=) && return 13
  f === (==) && return 14
  f === (!=) && return 15
  -1
end
function _unary_code(f)
  (f === identity || f === (+)) && return 0   # no op
  f === (-) && return 6
  f === abs && return 7
  f === abs2 && return 8
  f === conj && return 9
  -1
end

# scalar kind as _bcast_scalar types it
# (3: a value of real(T) next to complex vectors, Julia's Real ∘ Complex methods)
_expr_kind(::Type{T}, a::Float64) where {T} = 1
_expr_kind(::Type{T}, a::Float64) where {T<:Complex} = 1
_expr_kind(::Type{T}, a::ComplexF64) where {T<:Complex} = 2
_expr_kind(::Type{T}, a::Real) where {T<:Complex} = 3
_expr_kind(::Type{T}, a) where {T} = 0

# (wide, real valued) of an operand, or nothing when the tree is not supported
_expr_type(::Type{T}, a::HIPVector{T}) where {T} = (false, !(T <: Complex))
_expr_type(::Type{T}, a::HIPVector) where {T} = nothing   # mixed element types
function _expr_type(::Type{T}, a::Number) where {T}
  k = _expr_kind(T, a)
  k == 0 && T <: Real && !(a isa Real) && return nothing   # host path raises the InexactError
  (k == 1 || k == 2, !(T <: Complex) || k == 1 || k == 3)
end
function _expr_type(::Type{T}, b::HIPBroadcasted) where {T}
  ts = map(a -> _expr_type(T, a), b.args)
  any(t -> t === nothing, ts) && return nothing
  wide = any(t -> t[1], ts)
  allreal = all(t -> t[2], ts)
  if length(b.args) == 1
    c = _unary_code(b.f)
    (c < 0 || (c == 7 && !allreal)) && return nothing
    return (wide, allreal || c == 8)
  end
  length(b.args) == 2 || return nothing
  c = _binary_code(b.f)
  c < 0 && return nothing
  (c == 5 || 10 <= c <= 13) && !allreal && return nothing   # complex division, ordered comparison
  (wide && c < 10, allreal || c >= 10)   # a comparison's Bool takes the other operand's type
end

_expr_need(a::HIPVector) = 1
_expr_need(a::Number) = 0
function _expr_need(b::HIPBroadcasted)
  n = map(_expr_need, b.args)
  (length(n) == 1 || 0 in n) && return max(maximum(n), 1)
  n[1] >= n[2] ? max(n[1], n[2] + 1) : max(n[2], n[1] + 1)
end

function _expr_tags(::Type{T}, a) where {T}
  t = _expr_type(T, a)
  (t[1] ? PA_EXPR_WIDE : 0x00) | ((T <: Complex && t[2]) ? PA_EXPR_LREAL : 0x00)
end

function _expr_scalar!(e::ExprEncoder, ::Type{T}, a) where {T}
  k = _expr_kind(T, a)
  v = k == 0 ? T(a) : k == 3 ? real(T)(a) : a
  slot = zeros(UInt8, 16)
  GC.@preserve slot unsafe_store!(convert(Ptr{typeof(v)}, pointer(slot)), v)
  for j in eachindex(e.kinds)
    e.kinds[j] == k && e.scal[16j-15:16j] == slot && return UInt8(j - 1)
  end
  append!(e.scal, slot)
  push!(e.kinds, Cint(k))
  UInt8(length(e.kinds) - 1)
end

function _expr_push!(e::ExprEncoder, op::PaExprOp)
  push!(e.ops, op)
  e.sp += 1
  e.depth = max(e.depth, e.sp)
end

function _expr_emit!(e::ExprEncoder, ::Type{T}, a::HIPVector) where {T}
  k = findfirst(v -> v === a, e.vecs)
  if k === nothing
    push!(e.vecs, a)
    k = length(e.vecs)
  end
  _expr_push!(e, PaExprOp(0x00, UInt8(k - 1), 0x00, 0x00))
end
_expr_emit!(e::ExprEncoder, ::Type{T}, a::Number) where {T} =
  _expr_push!(e, PaExprOp(0x01, _expr_scalar!(e, T, a), _expr_tags(T, a), 0x00))
function _expr_emit!(e::ExprEncoder, ::Type{T}, b::HIPBroadcasted) where {T}
  if length(b.args) == 1
    _expr_emit!(e, T, b.args[1])
    c = _unary_code(b.f)
    c == 0 || push!(e.ops, PaExprOp(UInt8(c), 0x00, _expr_tags(T, b.args[1]), 0x00))
    return
  end
  l, r = b.args
  tl, tr = _expr_tags(T, l), _expr_tags(T, r)
  fl = ((tl | tr) & PA_EXPR_WIDE) | (tl & PA_EXPR_LREAL) | ((tr & PA_EXPR_LREAL) != 0 ? PA_EXPR_RREAL : 0x00)
  c = UInt8(_binary_code(b.f))
  if r isa Number
    _expr_emit!(e, T, l)
    push!(e.ops, PaExprOp(c, _expr_scalar!(e, T, r), fl | PA_EXPR_SC, 0x00))
  elseif l isa Number
    _expr_emit!(e, T, r)
    push!(e.ops, PaExprOp(c, _expr_scalar!(e, T, l), fl | PA_EXPR_CS, 0x00))
  else
    first_left = _expr_need(l) >= _expr_need(r)
    _expr_emit!(e, T, first_left ? l : r)
    _expr_emit!(e, T, first_left ? r : l)
    e.sp -= 1
    push!(e.ops, PaExprOp(c, 0x00, fl | (first_left ? PA_EXPR_SS : PA_EXPR_RS), 0x00))
  end
  nothing
end

# (PaExpr, encoder, root is real valued) or nothing
function _expr_encode(::Type{T}, root::HIPArg) where {T<:DeviceEltype}
  t = _expr_type(T, root)
  t === nothing && return nothing
  e = ExprEncoder(Any[], UInt8[], Cint[], PaExprOp[], 0, 0)
  _expr_emit!(e, T, root)
  (length(e.ops) > PA_EXPR_MAX_OPS || e.depth > PA_EXPR_MAX_DEPTH || length(e.vecs) > PA_EXPR_MAX_VECS ||
   length(e.kinds) > PA_EXPR_MAX_SCALARS) && return nothing
  nul = PaExprOp(0x00, 0x00, 0x00, 0x00)
  ops = ntuple(i -> i <= length(e.ops) ? e.ops[i] : nul, 32)
  (PaExpr(Int32(length(e.ops)), ops), e, t[2])
end

_expr_eltype(a::HIPVector{T}) where {T<:DeviceEltype} = T
_expr_eltype(a) = nothing
function _expr_eltype(b::HIPBroadcasted)
  for a in b.args
    T = _expr_eltype(a)
    T === nothing || return T
  end
  nothing
end

# ghosts are computed only when every vector operand shares one rows object (Interfaces.jl:1730)
_expr_shared(a, rows) = true
_expr_shared(a::HIPVector, rows) = a.rows === rows
_expr_shared(b::HIPBroadcasted, rows) = all(a -> _expr_shared(a, rows), b.args)

function _expr_eval!(y::HIPVector{T}, prog, bc::HIPArg) where {T<:DeviceEltype}
  expr, e, _ = prog
  all_lids = _expr_shared(bc, y.rows)
  all_lids || @assert all(v -> oids_are_equal(y.rows, v.rows), e.vecs)
  aliased = any(v -> v === y, e.vecs)
  vh = map(dev_vec, e.vecs)
  ih = map(v -> dev_idx(v.rows), e.vecs)
  yv = (all_lids && !aliased) ? dev_vec_nocopy(y) : dev_vec(y)   # owned only: y's ghosts are kept
  iy = dev_idx(y.rows)
  ns = length(e.kinds)
  for i in eachindex(yv)
    vi = Ptr{Cvoid}[h[i] for h in vh]
    ii = Ptr{Cvoid}[h[i] for h in ih]
    check(ccall((:pa_vec_eval, libpa), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ref{PaExpr}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Ptr{UInt8},
                 Ptr{Cint}, Cint),
                yv[i], iy[i], Ref(expr), Cint(length(vi)), vi, ii, Cint(ns), e.scal, e.kinds, all_lids ? 1 : 0))
  end
  mark_device_newer!(y)
end

# the tree reduced over the owned values (kind PA_REDUCE_*), or nothing when
# it is not supported; SUM: a T, MAX / MIN: a Float64
function _expr_reduce(::Type{T}, kind::Cint, bc::HIPArg) where {T<:DeviceEltype}
  prog = _expr_encode(T, bc)
  prog === nothing && return nothing
  expr, e, isreal = prog
  (kind == PA_REDUCE_SUM || isreal) || return nothing
  vh = map(dev_vec, e.vecs)
  ih = map(v -> dev_idx(v.rows), e.vecs)
  n = length(vh[1])
  vflat = Ptr{Cvoid}[h[i] for i in 1:n for h in vh]
  iflat = Ptr{Cvoid}[h[i] for i in 1:n for h in ih]
  r = Ref{ComplexF64}(0)   # 16 bytes: a T (SUM) or a Float64 (MAX / MIN) at offset 0
  check(ccall((:pa_reduce_expr_all, libpa), Cint,
              (Cint, Cint, Ref{PaExpr}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, Ptr{UInt8}, Ptr{Cint},
               Ref{ComplexF64}),
              n, kind, Ref(expr), Cint(length(e.vecs)), vflat, iflat, Cint(length(e.kinds)), e.scal, e.kinds, r))
  S = kind == PA_REDUCE_SUM ? T : Float64
  v = GC.@preserve r unsafe_load(convert(Ptr{S}, Base.unsafe_convert(Ptr{ComplexF64}, r)))
  (kind == PA_REDUCE_SUM && isreal) ? real(v) : v
end

_expr_node(f, args...) = HIPBroadcasted(f, args, _rows(first(a for a in args if a isa HIPArg)))

# sum of a tree (Interfaces.jl:1973-1983 over the broadcast's values)
function Base.sum(bc::HIPBroadcasted)
  T = _expr_eltype(bc)
  r = T === nothing ? nothing : _expr_reduce(T, PA_REDUCE_SUM, bc)
  r === nothing ? sum(Base.materialize(bc)) : r
end

# == (Interfaces.jl:1682-1686): equal lengths, parts and owned values
function Base.:(==)(a::HIPVector{T}, b::HIPVector{T}) where {T<:DeviceEltype}
  length(a) == length(b) && num_parts(a.values) == num_parts(b.values) || return false
  map(num_oids, a.rows.partition.parts) == map(num_oids, b.rows.partition.parts) || return false
  _expr_reduce(T, PA_REDUCE_MIN, _expr_node(==, a, b)) > 0
end

# maximum / minimum, plain and mapped with abs / abs2 / identity
# (Interfaces.jl:1841-1863); any(f, v) / all(f, v) with a closure stay generic
const HIPMapped = Union{typeof(abs),typeof(abs2),typeof(identity)}
function _expr_extremum(f, a::HIPVector{T}, kind::Cint) where {T<:DeviceEltype}
  r = _expr_reduce(T, kind, _expr_node(f, a))
  r === nothing ? nothing : real(T)(r)
end
function Base.maximum(f::HIPMapped, a::HIPVector{T}) where {T<:DeviceEltype}
  r = _expr_extremum(f, a, PA_REDUCE_MAX)
  r === nothing ? invoke(maximum, Tuple{Function,PVector}, f, a) : r
end
function Base.minimum(f::HIPMapped, a::HIPVector{T}) where {T<:DeviceEltype}
  r = _expr_extremum(f, a, PA_REDUCE_MIN)
  r === nothing ? invoke(minimum, Tuple{Function,PVector}, f, a) : r
end
Base.maximum(a::HIPVector{T}) where {T<:Union{Float32,Float64}} = maximum(identity, a)
Base.minimum(a::HIPVector{T}) where {T<:Union{Float32,Float64}} = minimum(identity, a)

# Distances (Interfaces.jl:1774-1817): Σ |a - b|² in one pass
function (d::Distances.SqEuclidean)(a::HIPVector{T}, b::HIPVector{T}) where {T<:DeviceEltype}
  @assert oids_are_equal(a.rows, b.rows)
  real(sum(_expr_node(abs2, _expr_node(-, a, b))))
end
(d::Distances.Euclidean)(a::HIPVector{T}, b::HIPVector{T}) where {T<:DeviceEltype} =
  sqrt(Distances.SqEuclidean()(a, b))

_host_arg(a) = a
_host_arg(a::HIPBroadcasted) = _host_broadcasted(a)
function _host_broadcasted(bc::HIPBroadcasted)
  args = map(_host_arg, bc.args)
  # the generic methods (map_parts syncs the parts that are newer on the device)
  if length(args) == 2 && args[1] isa Number
    invoke(Base.broadcasted, Tuple{Any,Number,Union{PVector,PartitionedArrays.DistributedBroadcasted}}, bc.f, args...)
  elseif length(args) == 2 && args[2] isa Number
    invoke(Base.broadcasted, Tuple{Any,Union{PVector,PartitionedArrays.DistributedBroadcasted},Number}, bc.f, args...)
  else
    invoke(Base.broadcasted, Tuple{Any,Vararg{Union{PVector,PartitionedArrays.DistributedBroadcasted}}}, bc.f, args...)
  end
end

# ---- Jacobi preconditioner (DESIGN.md §4.11) --------------------------------
# diag(A) read off the device layout (pa_mat_diag: no entry table, no nzval
# download), ghosts exchanged from their owners, and P = HIPJacobi(A) with
# ldiv!(c, P, r) on the device, so IterativeSolvers.cg!(x, A, b; Pl=P) — the
# generic iterate, see below — runs on device operations.  Float32 / Float64.
const PcgEltype = Union{Float32,Float64}
function LinearAlgebra.diag(A::HIPMatrix{T}) where {T<:PcgEltype}
  oids_are_equal(A.rows, A.cols) || error("diag: A.rows and A.cols own different ids")
  d = PVector{T}(undef, A.cols)
  M = dev_mat(A); R = dev_idx(A.rows); K = dev_idx(A.cols); D = dev_vec_nocopy(d)
  for i in eachindex(M)
    check(ccall((:pa_mat_diag, libpa), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                M[i], R[i], K[i], D[i]))
  end
  mark_device_newer!(d)
  PartitionedArrays.exchange!(d)
  d
end
struct HIPJacobi{V}
  d::V   # the diagonal on every lid (a HIPVector on the solve's PRange)
end
HIPJacobi(A::PSparseMatrix) = HIPJacobi(diag(A))
function LinearAlgebra.ldiv!(c::HIPVector{T}, P::HIPJacobi, r::HIPVector{T}) where {T<:PcgEltype}
  (c.rows === r.rows && r.rows === P.d.rows) || error("ldiv!(c, ::HIPJacobi, r): one PRange for c, r and the diagonal")
  rho = Ref{T}(zero(T))
  check(ccall((:pa_pcg_apply_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ref{T}),
              num_parts(c.values), dev_vec_nocopy(c), dev_vec(r), dev_vec(P.d), dev_idx(c.rows), rho))
  mark_device_newer!(c)
  c
end
# x .+= α.*u; r .-= α.*c; c = P \ r in one pass: (norm(r), dot(c, r)) of the new values
function pcg_update!(x::HIPVector{T}, r::HIPVector{T}, u::HIPVector{T}, c::HIPVector{T}, P::HIPJacobi,
                     α::Number) where {T<:PcgEltype}
  a = Ref{T}(T(α)); rho = Ref{T}(zero(T)); res = Ref{Float64}(0.0)
  check(ccall((:pa_pcg_update_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
               Ptr{Ptr{Cvoid}}, Ref{T}, Ref{Float64}, Ref{T}),
              num_parts(x.values), dev_vec(x), dev_vec(r), dev_vec(u), dev_vec(c), dev_vec(P.d),
              dev_idx(x.rows), a, res, rho))
  mark_device_newer!(x); mark_device_newer!(r); mark_device_newer!(c)
  res[], rho[]
end

# every part's owned lids are 1..num_oids (the layout the fused reductions ride on)
_own_contig(r::PRange) =
  all(s -> collect(s.oid_to_lid) == collect(1:length(s.oid_to_lid)), r.partition.parts)

# ---- IterativeSolvers.cg! (v0.9) with the recurrence on the device --------
# (pa_cg_solve_all: the same iterates as the generic cg! over the
# specialisations above, bit for bit, with no host round trip per iteration)
# log = true returns IterativeSolvers' ConvergenceHistory: that keeps the
# generic cg! (over the specialisations above); verbose is not printed here.
# Pl = HIPJacobi(A) with a real T, no log, no statevars and a range whose
# owned lids are contiguous runs the
# preconditioned recurrence on the device as well (pa_pcg_solve_all: the
# iterates of the generic cg! over ldiv!(c, Pl, r), dot, mul! and the
# broadcasts above, with ρ, β, α of type T).  Any other Pl keeps the generic
# cg!, whose operations on HIP vectors are still the device ones.
function IterativeSolvers.cg!(x::HIPVector{T}, A::HIPMatrix{T}, b::HIPVector{T};
                              abstol::Real=zero(real(T)), reltol::Real=sqrt(eps(real(T))),
                              maxiter::Int=size(A, 2), log::Bool=false, initially_zero::Bool=false,
                              kwargs...) where {T<:DeviceEltype}
  Pl = get(kwargs, :Pl, nothing)
  # pa_pcg_solve_all needs owned lids 1..num_oids on every part; other ranges
  # (with_ghost, periodic) keep the generic iterate, as before
  jacobi = Pl isa HIPJacobi && T <: PcgEltype && length(kwargs) == 1 && _own_contig(x.rows)
  if log || haskey(kwargs, :statevars) || !(Pl === nothing || jacobi)
    return invoke(IterativeSolvers.cg!, Tuple{Any,Any,Any}, x, A, b; abstol=abstol, reltol=reltol,
                  maxiter=maxiter, log=log, initially_zero=initially_zero, kwargs...)
  end
  u, r, c = similar(x), similar(x), similar(x)
  bb = b.rows === x.rows ? b : copyto!(similar(x), b)
  its = Ref{Int64}(0); res = Ref{Float64}(0.0)
  if jacobi
    d = Pl.d.rows === x.rows ? Pl.d : PartitionedArrays.exchange!(copyto!(similar(x), Pl.d))
    check(ccall((:pa_pcg_solve_all, libpa), Cint,
                (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
                 Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
                 Float64, Float64, Int64, Cint, Ref{Int64}, Ref{Float64}, Ptr{Float64}),
                num_parts(x.values), dev_mat(A), dev_vec(x), dev_vec(bb), dev_vec(d), dev_vec_nocopy(u),
                dev_vec_nocopy(r), dev_vec_nocopy(c), dev_idx(x.rows), dev_xchg(x.rows),
                Float64(reltol), Float64(abstol), maxiter, Cint(16), its, res, Ptr{Float64}(C_NULL)))
    mark_device_newer!(x)
    return x
  end
  check(ccall((:pa_cg_solve_all, libpa), Cint,
              (Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
               Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
               Float64, Float64, Int64, Cint, Ref{Int64}, Ref{Float64}, Ptr{Float64}),
              num_parts(x.values), dev_mat(A), dev_vec(x), dev_vec(bb), dev_vec_nocopy(u),
              dev_vec_nocopy(r), dev_vec_nocopy(c), dev_idx(x.rows), dev_xchg(x.rows),
              Float64(reltol), Float64(abstol), maxiter, Cint(16), its, res, Ptr{Float64}(C_NULL)))
  mark_device_newer!(x)
  x
end

end # module

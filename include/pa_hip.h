/*
 * pa_hip.h — C-ABI of the MI355X-native backend for PartitionedArrays.jl's
 * SpMV + halo hot path (libpa_hip.so).
 *
 * This is the drop-in boundary.  A Julia `HIPBackend <: AbstractBackend`
 * binds these symbols with `ccall`; the Python host
 * package in partitionedarrays.jl_amd/ binds them with ctypes and is the
 * stand-in for that shim in this repository (no Julia on this image).
 *
 * Conventions:
 *  - every entry point returns int: 0 = ok, <0 = error; the message of the
 *    last error of the calling thread is in pa_last_error();
 *  - all index inputs are Julia 1-based (Int32 unless a width is passed);
 *    they are converted once, at create time;
 *  - the library copies host inputs and owns all device memory; handles are
 *    opaque and freed by their *_destroy;
 *  - a process holds one or more parts ("local parts"); the *_all entry
 *    points take the arrays of handles of all local parts, in part order,
 *    mirroring `map_parts` over an AbstractPData.  Neighbours held by the
 *    same process are served by device copies, neighbours in other processes
 *    by RCCL point-to-point over xGMI (after pa_comm_init_rank);
 *  - dtype codes: PA_F32, PA_F64, PA_C64 (ComplexF32), PA_C128 (ComplexF64).
 *    Scalars (alpha, beta, results) are passed as pointers to host values of
 *    the vector's element type;
 *  - threading: one host thread drives a set of parts (the reference's
 *    tasks run on the main Julia task too); the library may issue a call's
 *    per-part work from its own threads.  The tuning knobs are resolved per
 *    call (the process defaults of pa_tune under the call's context
 *    overrides, pa_ctx_tune) and never written while a call runs, so calls
 *    on different parts from different host threads each run with their own
 *    context's knobs (pa_knob_selftest).  The per-context caches are not
 *    synchronised: concurrent calls must not share a context.
 *    pa_last_error is per thread.
 */
#ifndef PA_HIP_H
#define PA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PA_F32 = 0, PA_F64 = 1, PA_C64 = 2, PA_C128 = 3 };
enum { PA_REPLACE = 0, PA_ADD = 1 };

typedef struct pa_ctx pa_ctx;
typedef struct pa_index pa_index;
typedef struct pa_xchg pa_xchg;
typedef struct pa_vec pa_vec;
typedef struct pa_mat pa_mat;
typedef struct pa_coo pa_coo;
typedef struct pa_table pa_table; /* one part's Table: rows of any length */
typedef struct pa_event pa_event; /* completion of one call's work for one part */

/* ---- errors / library info ------------------------------------------- */
const char* pa_last_error(void);
int pa_version(void);
/* number of visible HIP devices (0 when no GPU). */
int pa_device_count(int* count);
/* Process-wide tuning knobs (performance only, results unchanged); each is
 * an A/B lever kept because a configuration uses it or a test pins it:
 * "spmv_flags"  bit 0: non-temporal value/column streams, bit 1: pattern
 *               and triple-SELL slices read their offset, length and mask /
 *               ghost base as one descriptor load, bit 2: pattern
 *               rows fetch x as 16 B runs, bit 3: the last len % U entries
 *               of a slice as one predicated batch, bit 4: a slice list
 *               covering the whole structure is launched without the list,
 *               bit 5: y written with non-temporal stores, bit 6: launches
 *               whose rows have at most 8 entries use the short-row kernels
 *               (one predicated batch, no loop: fewer registers), bit 7:
 *               the Float64 short-row tail launch of rows <= 7 entries at
 *               7 waves per SIMD (default 223);
 * "spmv_format" 1: pattern slices where the matrix has them (default),
 *               0: int32 column ids everywhere;
 * "long_rows_exact" 1: long rows summed in the reference's order (default),
 *               0: lane-strided partial sums + tree (within 1e-12);
 * "halo_pull"   1: parts of one process read their neighbours' packed
 *               buffers directly (default), 0: staging copies;
 * "spmv_delta16" 1: int32-column slices whose columns fit 16-bit codes
 *               store those (matrices built afterwards; default), 0: off;
 * "spmv_merge"  1: every slice kind of every part of a mul! without a halo
 *               in flight as one launch (default), 0: one launch per kind;
 * "spmv_merge_max" parts with more slices than this run one launch per
 *               kind (default 65536; 0: no limit);
 * "halo_direct" 1: mul! over parts sharing a stream pair reads every ghost
 *               straight from its owner's x on the compute stream (no
 *               pack, no cross-stream event; default), 0: pack + pull on
 *               the comm stream overlapped with the interior slices.  The
 *               direct pull reads the senders' x while it writes the
 *               receivers', so it is taken only when no part of the call
 *               sends a lid that it also receives (true of every exchanger
 *               made from a PRange: owned lids sent, ghosts received);
 *               otherwise the call packs first, as with 0.  An exchanger
 *               that receives on owned lids also makes mul! run the interior
 *               slices after the halo instead of beside it;
 * "halo_transport" 0 (default): parts of one process exchange by device
 *               reads/copies, except parts whose communicator came from
 *               pa_comm_init_all (RCCL, per context); 1: RCCL send/recv for
 *               every part that has a communicator;
 * "cg_fuse"     0: the device CG's u .= r .+ beta.*u as its own sweep,
 *               1: inside the SpMV (XV kernels), 2 (default, auto): with
 *               all parts in one process and at least three batches, one
 *               batch of each, then the faster (remembered on the matrix);
 *               otherwise the sweep or the matrix's earlier choice;
 * "spmv_group"  1: the parts of one process sharing a stream pair run each
 *               mul! phase as one launch (default), 0: launches per part;
 * "pattern_min_regular" a slice becomes a pattern slice when at least this
 *               percentage of its rows follow its pattern (1-100; 0 = auto,
 *               the default: 70, 50 for Float32's 256-row slices; matrices
 *               built afterwards), the others go to the side SELL;
 * "issue_threads" a mul! over several parts with their own stream pairs is
 *               issued from host threads, one part per thread: 1 when the
 *               parts span several devices (default), 2 always, 0 never
 *               (the calling thread, one part after the other);
 * "halo_barrier" 1: such a mul! (local neighbours) waits for one pack
 *               barrier per call and alternates two send buffers (default),
 *               0: per-neighbour event waits before every pack and pull;
 * "spmv_tri16"  the triple SELL for delta16 slices (see below): 1 for
 *               slices of 1-2 rows per lane (default), 0 never;
 * "spmv_tri_order" 1: its other rows first (default), 0: triple rows first;
 * "spmv_xcd_chunk" -1 (default, auto): one-launch-per-kind calls run their
 *               workgroups in runs of (pattern reach / 8) blocks per XCD,
 *               merged launches round robin; C > 0: runs of C; 0: round robin;
 * "spmv_side_tail" 1: per-kind launches run short side rows as the pattern
 *               launch's trailing waves (default), 0: their own launch;
 * "f32_rows"    Float32 SELL rows per lane (matrices built afterwards):
 *               4 (16 B value packs, 256-row slices), 2 (8 B packs, 128-row
 *               slices: the Float64 geometry, so delta16 rows take the
 *               triple SELL), 0 (default, auto): 4, rebuilt with 2 when
 *               fewer than 80 % of the slices are pattern slices;
 * "spmv_tri_pack" triple-SELL slices of 2 rows per lane (matrices built
 *               afterwards): bit 2 pair slices (every element type,
 *               pa_mat_pair_info), bit 0 their Float32 values as one 16 B
 *               and one 8 B pack per triple and lane (bit 1 unused);
 *               7 (default), 0 none;
 * "spmv_uniform" 1 (default): Float64 pattern slices whose patterns (<= 7
 *               entries) are subsequences of one union U (FD7) also keep
 *               their values at slice * H * |U| in U's order, so the
 *               short-row tail launch issues its loads before the slice's
 *               descriptor arrives (matrices built afterwards); 0 off;
 * "scatter_wide" 0 (default): pa_vec_scatter sorts 32-bit keys and payloads
 *               when the part's lids and the entries fit them, 1: always the
 *               64-bit ones;
 * "fault_inject" tests only: threaded issue jobs add an invalid launch. */
int pa_tune(const char* key, int value, int* previous);
/* The same knobs for one context: calls led by parts of `c` (their first
 * part's context) run with this value instead of the process default, for
 * the duration of the call; value PA_TUNE_DROP drops the override (a value
 * outside every knob's range: -1 is a valid value, spmv_xcd_chunk's auto).
 * *previous gets the context's former override (PA_TUNE_DROP: none).     */
#define PA_TUNE_DROP (-2147483647 - 1)
int pa_ctx_tune(pa_ctx* c, const char* key, int value, int* previous);
/* Test support (no device needed): `nthreads` host threads resolve calls'
 * knobs with different context overrides, on their own threads and on the
 * library's issue threads, while the process default changes; *mismatches
 * counts resolutions that saw another call's value (0 expected).        */
int pa_knob_selftest(int nthreads, int iters, int* mismatches);
/* HBM calibration of `device` (not the hot path): best read-only and copy
 * rates (GB/s, read+write bytes for the copy; best of 4/8 loads in flight
 * per lane and four grid sizes) over `reps` sweeps of a
 * `bytes` buffer with the SpMV's 16 B non-temporal loads.  bench.py reports
 * the SpMV's PMC-measured rate against it, since boxes differ.           */
int pa_hbm_probe(int device, int64_t bytes, int reps, double* read_gbs, double* copy_gbs);
/* The same read sweep at the size of ONE launch: every launch reads
 * `bytes_per_launch` (one operator's bytes), the launches rotating over
 * `span` bytes (>= 1 GiB: from HBM, not the 256 MB Infinity Cache), so the
 * rate includes one launch's ramp-up and drain; best of the grid sizes.  A
 * short SpMV (C2's 149 MB) is compared with this, not with the sweep of a
 * large buffer.                                                           */
int pa_hbm_probe_launch(int device, int64_t bytes_per_launch, int64_t span, int reps, double* read_gbs);

/* ---- part context ------------------------------------------------------
 * One context per part: its device, its streams, its scratch.
 * Replaces the part slot of `get_part_ids(b::AbstractBackend, nparts)`
 * (Interfaces.jl:24) — part is 1-based, 1 <= part <= nparts.          */
int pa_ctx_create(int device, int part, int nparts, pa_ctx** out);
/* A context for another part on `with`'s device that shares its stream
 * pair: several parts of one process on one GPU then form a single
 * in-order chain (no cross-stream events between them).                 */
int pa_ctx_create_shared(int part, int nparts, pa_ctx* with, pa_ctx** out);
int pa_ctx_destroy(pa_ctx* ctx);
int pa_ctx_sync(pa_ctx* ctx);

/* RCCL bootstrap for the one-part-per-process mode (the MPIBackend role,
 * MPIBackend.jl:9-36): rank 0 makes the id, the host broadcasts it (MPI
 * Bcast / torch.distributed), every rank calls pa_comm_init_rank with
 * rank = part-1 and nranks = nparts.                                    */
int pa_comm_unique_id(unsigned char id[128]);
int pa_comm_init_rank(pa_ctx* ctx, const unsigned char id[128]);
/* RCCL between the parts of one process (ncclCommInitAll over the distinct
 * devices of ctx[0..n-1] = parts 1..nparts, in order: one rank per device,
 * in order of first appearance; parts of one device share its rank, and
 * must share their stream pair, so a segment between them is a send to
 * self).  Every halo segment of these contexts then moves by the same
 * grouped ncclSend/ncclRecv as across processes (MPIBackend.jl:261-309),
 * posted in (sender part, receiver part) order; contexts without it (or
 * not from pa_comm_init_all) read each other's buffers.                  */
int pa_comm_init_all(int n, pa_ctx* const ctx[]);
/* Halo bytes this part has posted to RCCL sends / receives so far (what the
 * grouped ncclSend/ncclRecv carried for it; 0 when every segment moved by
 * device reads).                                                          */
int pa_comm_stats(pa_ctx* ctx, int64_t* bytes_sent, int64_t* bytes_recv);
/* What this part's communicator runs on, so that a multi-process run can
 * show it (the reference asserts Comm_size == prod(nparts),
 * MPIBackend.jl:11,17,61): *ranks = ncclCommCount (0: no communicator),
 * *rank = ncclCommUserRank, the context's device ordinal and its PCI bus id
 * (pci, >= 16 bytes: distinct GPUs of a node have distinct ids), the RCCL
 * version (ncclGetVersion) and the path of the librccl the process resolved
 * it from (lib, lib_len bytes; dladdr on ncclGetVersion: a host that loads
 * another RCCL first, e.g. torch's bundled one, shows it here).          */
/* Host time of the library's issue jobs (one part's share of a call issued
 * from an IssuePool thread: its runtime calls and launches) since the last
 * reset: the largest and the mean job, and their count.  The per-thread
 * issue time of one process driving several GPUs.         */
int pa_issue_stats(int reset, double* max_job_us, double* mean_job_us, int64_t* jobs);
int pa_comm_info(pa_ctx* ctx, int* ranks, int* rank, int* device, char* pci, int pci_len, int* version,
                 char* lib, int lib_len);

/* ---- index sets --------------------------------------------------------
 * Device copy of an AbstractIndexSet's oid_to_lid / hid_to_lid
 * (IndexSets.jl:215-265, 343-421).  1-based Int32 inputs.  Contiguous
 * layouts (oid_to_lid == 1:noids, hid_to_lid == noids+1:nlids) are detected
 * and kept as ranges (no device table).                                  */
int pa_index_create(pa_ctx* ctx, int64_t nlids,
                    int64_t noids, const int32_t* oid_to_lid,
                    int64_t nhids, const int32_t* hid_to_lid,
                    pa_index** out);
int pa_index_destroy(pa_index* idx);

/* ---- exchanger (halo plan) ----------------------------------------------
 * `Exchanger{parts_rcv,parts_snd,lids_rcv,lids_snd}` (Interfaces.jl:698-713)
 * verbatim: parts_* are 1-based part ids, ptrs_* are the 1-based Table ptrs
 * (length n+1), lids_* the 1-based Table data.                            */
int pa_xchg_create(pa_ctx* ctx,
                   int32_t n_rcv, const int32_t* parts_rcv,
                   const int32_t* ptrs_rcv, const int32_t* lids_rcv,
                   int32_t n_snd, const int32_t* parts_snd,
                   const int32_t* ptrs_snd, const int32_t* lids_snd,
                   pa_xchg** out);
int pa_xchg_destroy(pa_xchg* xg);

/* Global ids on the device.
 * pa_index_set_gids: attach lid_to_gid (num_lids 1-based gids) to the
 * index set; the library keeps a sorted gid → lid table on the device.
 * pa_add_gids: add_gids!(a, gids) (Interfaces.jl:579-603, 618-627) — the
 * n gids that are not local ids of the set, each once, in first-touch order,
 * into new_gids (capacity cap; *n_new is set even when it exceeds cap, and
 * the call then fails so the caller can retry).  The host appends them as
 * ghosts with their owners (gid_to_part) and builds the Exchanger.       */
int pa_index_set_gids(pa_index* idx, const int64_t* lid_to_gid);
int pa_add_gids(pa_index* idx, int64_t n, const int64_t* gids, int64_t cap,
                int64_t* new_gids, int64_t* n_new);
/* to_lids!(ids, a) (Interfaces.jl:1541-1543, IndexSets.jl gid_to_lid): the
 * n 1-based gids in ids become 1-based lids, in place, through the device
 * gid table; a gid that is not a local id fails (KeyError).  Exchanger
 * (Interfaces.jl:723-786) uses it for lids_snd of the gids its receivers
 * asked for.                                                              */
int pa_index_to_lids(pa_index* idx, int64_t n, int64_t* ids);
/* to_gids!(ids, a) (Interfaces.jl:638-645, 1545-1547), the mirror of
 * pa_index_to_lids: the n 1-based lids in ids become 1-based gids, in place,
 * through the lid_to_gid that pa_index_set_gids attached (kept on the device,
 * 8 B per lid).  A lid outside 1..num_lids fails (BoundsError) and nothing
 * is written.                                                             */
int pa_index_to_gids(pa_index* idx, int64_t n, int64_t* ids);

/* ---- vectors (the values of one part of a PVector) --------------------- */
int pa_vec_create(pa_ctx* ctx, int dtype, int64_t n, pa_vec** out);
int pa_vec_destroy(pa_vec* v);
int pa_vec_upload(pa_vec* v, const void* host, int64_t n);
int pa_vec_download(const pa_vec* v, void* host, int64_t n);
/* the device address of v's values (lid 1 at offset 0; valid until
 * pa_vec_destroy): zero-copy interop, e.g. Julia's unsafe_wrap of a
 * ROCArray over a part's values, and placement diagnostics              */
int pa_vec_device_ptr(const pa_vec* v, void** out);
/* fill!(v, s) (Interfaces.jl:1966-1971), all lids */
int pa_vec_fill(pa_vec* v, const void* s);
/* copyto!(dst, src): all lids when same_layout, owned values otherwise
 * (Interfaces.jl:1659-1667).  idx_* describe each vector's partition.    */
int pa_vec_copy(pa_vec* dst, const pa_index* idx_dst,
                const pa_vec* src, const pa_index* idx_src, int same_layout);
/* Fused broadcast kernels for the CG recurrence (Interfaces.jl:1710-1737),
 * evaluated exactly as Julia's scalar loop (no FMA contraction):
 *   mode 0: y[i] = x[i] + a*y[i]     (u .= r .+ β.*u)
 *   mode 1: y[i] = y[i] + a*x[i]     (x .+= α.*u)
 *   mode 2: y[i] = y[i] - a*x[i]     (r .-= α.*c)
 *   mode 3: y[i] = y[i] - x[i]       (r .-= c)
 *   mode 4: y[i] = a*y[i]            (rmul!, Interfaces.jl:1675)
 * over all lids when all_lids != 0 (same partition: ghosts too), else over
 * the owned values through idx, which must describe both vectors: the same
 * lid layout, not merely equal owned ids (x is read at y's lids; vectors of
 * equal owned ids in another lid order, or next to other ghosts, take
 * pa_vec_eval, which has one index set per operand).
 * The scalar a is of the element type, or — mode | PA_BCAST_F64 — a
 * Float64 (double), or — mode | PA_BCAST_C128 — a ComplexF64 (complex
 * vectors only): then each element is evaluated in Float64 / ComplexF64
 * (Real * Complex componentwise) and rounded to the element type once,
 * Julia's promotion for e.g. IterativeSolvers' Float64 α, β with Float32
 * vectors.                                                                */
#define PA_BCAST_F64 8
#define PA_BCAST_C128 16
int pa_vec_axpby(pa_vec* y, const pa_vec* x, const pa_index* idx,
                 const void* a, int mode, int all_lids);

/* ---- COO constructor and indexed views of a PVector ----------------------
 * pa_vec_scatter: the n pairs (I[k], V[k]) written into the values of one
 * part, in input order.  With op PA_SCATTER_ADD and zero_first = 1 it is the
 * loop of PVector(init, I, V, rows; ids) (Interfaces.jl:1887-1910): the
 * values are filled with zero(T) over all lids (1901), then
 * values[lid] += V[k] for k = 1..n (1902-1905) — a single -0.0 entry gives
 * +0.0; with zero_first = 0 it is the batched `view[I] .+= V` on
 * local_view / global_view (test_fem_sa.jl:86-101), and op PA_SCATTER_SET
 * their setindex! (2027-2031, 2066-2069): the last entry of an id in input
 * order stays.  The result equals the sequential loop bit for bit whatever
 * the duplicates: the pairs are sorted stably by lid and each lid's entries
 * are added to it in input order by one thread, with plain adds (complex
 * values componentwise), no atomics.
 * ids_kind PA_IDS_LOCAL: I holds 1-based lids of idx (index_bytes 4 or 8); an
 * id outside 1..num_lids is an error (BoundsError).  PA_IDS_GLOBAL: I holds
 * 1-based Int64 gids (index_bytes 8), looked up in the gid table of idx
 * (pa_index_set_gids) and overwritten in place by the 1-based lids, as
 * to_lids! does in the constructor (1886, 1895-1897; visible in the sequence
 * test_interfaces.jl:501-503); a gid that is not a local id is an error
 * (KeyError).  Every id is checked before the first write: a failed call
 * leaves v and I unchanged.  idx must be the index set of v (num_lids = the
 * vector's length).  n = 0 and parts without lids are legal.
 * on_device = 1: I and V (pa_vec_gather: I and out) are device arrays on the
 * context's device — a ROCArray of the Julia caller, next to
 * pa_vec_device_ptr; otherwise host arrays, consumed before the call
 * returns.  The work is enqueued on the part's compute stream, ordered with
 * the part's other work.
 * pa_vec_gather: out[k] = v[lid of I[k]], getindex of the views.  An absent
 * global id reads zero(T) when absent_zero = 1 (LocalView, 2019-2026) and is
 * an error (KeyError) when 0 (GlobalView, 2062-2065); a local id out of range
 * is always an error.  I is left unchanged.                                 */
#define PA_IDS_LOCAL 0   /* 1-based lids of idx */
#define PA_IDS_GLOBAL 1  /* 1-based Int64 gids; needs pa_index_set_gids */
#define PA_SCATTER_ADD 0
#define PA_SCATTER_SET 1
int pa_vec_scatter(pa_vec* v, pa_index* idx, int ids_kind, int index_bytes,
                   int op, int zero_first, int on_device,
                   int64_t n, void* I, const void* V);
int pa_vec_gather(const pa_vec* v, pa_index* idx, int ids_kind, int index_bytes,
                  int absent_zero, int on_device,
                  int64_t n, const void* I, void* out);

/* ---- broadcast expressions (Interfaces.jl:1688-1765) --------------------
 * Any elementwise expression over PVectors and numbers as one pass: a
 * postfix program over at most PA_EXPR_MAX_VECS vector operands and
 * PA_EXPR_MAX_SCALARS scalars, at most PA_EXPR_MAX_OPS ops, evaluated per
 * element on an operand stack of PA_EXPR_MAX_DEPTH slots, then stored
 * (pa_vec_eval) or reduced (pa_reduce_expr_all).
 *
 * Op codes: PA_OP_VEC pushes element i of vector `arg`, PA_OP_SCAL pushes
 * scalar `arg`; the binary ops ADD SUB MUL DIV and the comparisons (1 or 0
 * of the node's type) take their operands as the mode bits of `flags` say:
 * PA_EXPR_SS below ∘ top (both popped), PA_EXPR_RS top ∘ below (the
 * reversed forms RSUB / RDIV: sibling subtrees are pure, so the encoder
 * emits the deeper one first and the depth stays minimal), PA_EXPR_SC
 * top ∘ scalar `arg`, PA_EXPR_CS scalar `arg` ∘ top (scalars as immediates:
 * no stack slot).  NEG ABS ABS2 CONJ replace the top.
 *
 * Types follow Julia's broadcast.  All vectors and y share one dtype T.
 * scalar_kinds[k]: 0 a value of T, 1 a Float64, 2 a ComplexF64 (complex T
 * only; into a real vector it is an InexactError), 3 a value of real(T) (an
 * Int or a Float32 next to ComplexF32 vectors: Julia's Real ∘ Complex
 * methods apply; with real T the same as 0); scalars holds one 16-byte
 * slot per scalar with the value of that type at offset 0.  A node is of T
 * unless an operand is a Float64 / ComplexF64 scalar or a wide node: then it
 * is of wide_of<T> (Float64 / ComplexF64) and its op carries PA_EXPR_WIDE;
 * a T op is evaluated in T, a wide op in the wide type, and the result is
 * rounded to T once on the store ((v .+ u) .* 2.0 with Float32 v, u adds in
 * Float32 and multiplies in Float64).  With complex T a node may be real
 * valued (a Float64 or real(T) scalar, abs2, a comparison): PA_EXPR_LREAL /
 * PA_EXPR_RREAL mark a real left / right operand (unary ops: LREAL), and the
 * op is Julia's Real ∘ Complex method (componentwise product, the imaginary
 * part kept by + and -).  DIV, ABS and the ordered comparisons take real
 * operands only; EQ and NE also complex ones.  A comparison's 1 / 0 is a
 * node of T whatever its operands' types (Julia's Bool takes the other
 * operand's type in arithmetic); its op still carries its operands' tags.  The tags must equal what
 * these rules infer (pa_expr_check), anything else is rejected.            */
#define PA_EXPR_MAX_OPS 32
#define PA_EXPR_MAX_VECS 8
#define PA_EXPR_MAX_SCALARS 8
#define PA_EXPR_MAX_DEPTH 4
enum { PA_OP_VEC = 0, PA_OP_SCAL = 1, PA_OP_ADD = 2, PA_OP_SUB = 3, PA_OP_MUL = 4, PA_OP_DIV = 5,
       PA_OP_NEG = 6, PA_OP_ABS = 7, PA_OP_ABS2 = 8, PA_OP_CONJ = 9, PA_OP_LT = 10, PA_OP_LE = 11,
       PA_OP_GT = 12, PA_OP_GE = 13, PA_OP_EQ = 14, PA_OP_NE = 15 };
enum { PA_EXPR_WIDE = 1, PA_EXPR_LREAL = 2, PA_EXPR_RREAL = 4,
       PA_EXPR_SS = 0, PA_EXPR_SC = 8, PA_EXPR_CS = 16, PA_EXPR_RS = 24, PA_EXPR_MODE = 24 };
enum { PA_REDUCE_SUM = 0, PA_REDUCE_MAX = 1, PA_REDUCE_MIN = 2 };
typedef struct pa_expr_op {
  uint8_t code;   /* PA_OP_* */
  uint8_t arg;    /* vector or scalar number */
  uint8_t flags;  /* PA_EXPR_WIDE | _LREAL | _RREAL | operand mode */
  uint8_t pad;    /* 0 */
} pa_expr_op;
typedef struct pa_expr {
  int32_t nops;
  pa_expr_op ops[PA_EXPR_MAX_OPS];
} pa_expr;
/* The checks pa_vec_eval / pa_reduce_expr_all run on a program before any
 * launch (no device needed): op codes, operand numbers, stack depth, the
 * type rules above.  *depth (optional) gets the stack depth the program
 * needs, *result_flags (optional) the root's PA_EXPR_WIDE / PA_EXPR_LREAL. */
int pa_expr_check(const pa_expr* prog, int dtype, int nvec, int nscal, const int* scalar_kinds,
                  int* depth, int* result_flags);
/* materialize!(y, bc) for one part (Interfaces.jl:1710-1720): y[i] =
 * prog(v[0][i], ..) over every lid when all_lids != 0 (every operand then
 * has y's length: the host passes it when all share y's partition object,
 * a.rows === b.rows at 1714 and 1730), else over the owned values, y and
 * each operand addressed through its own index set (equal owned counts;
 * ghosts of y untouched).  y may be one of the operands (same-index access).
 * Identity-addressed operands (all lids, or contiguous owned lids everywhere)
 * stream 16 B per lane and operand; otherwise one element per lane gathers
 * through the oid → lid tables.                                             */
int pa_vec_eval(pa_vec* y, const pa_index* y_idx, const pa_expr* prog, int nvec,
                const pa_vec* const v[], const pa_index* const v_idx[], int nscal,
                const void* scalars, const int* scalar_kinds, int all_lids);
/* The expression reduced over the owned values of the n local parts
 * (v[i * nvec + k], v_idx[i * nvec + k]: operand k of part i).
 * PA_REDUCE_SUM: sum(bc) as pa_sum_all (Interfaces.jl:1973-1983): Float64 /
 * ComplexF64 accumulator per part, each part's value rounded to T, parts
 * added in T in part order; result: host scalar of T.  PA_REDUCE_MAX / _MIN:
 * maximum / minimum (Interfaces.jl:1841-1863), real-valued expressions only,
 * init -Inf / +Inf (typemin / typemax; what a part without owned values
 * contributes), a NaN in any owned element gives NaN; result: host double.
 * With 0/1-valued expressions these are any / all (1827-1839), == (1682-1686),
 * and with abs / abs2 the norms and Distances metrics (1767-1817).          */
int pa_reduce_expr_all(int n, int kind, const pa_expr* prog, int nvec,
                       const pa_vec* const v[], const pa_index* const v_idx[], int nscal,
                       const void* scalars, const int* scalar_kinds, void* result);

/* ---- matrices (one part of a PSparseMatrix) ----------------------------
 * From the reference's local SparseMatrixCSC (1-based colptr/rowval with
 * index_bytes = 4 or 8, nzval of dtype), with the matrix's rows/cols index
 * sets.  Builds the owned-row split SELL layout once:
 * own-column entries in oid order, then ghost-column entries in hid order,
 * i.e. the summation order of SparseUtils.jl:176-185 applied to the
 * owned_owned and owned_ghost blocks (Interfaces.jl:2142-2156, 2261-2272).
 * Stored entries of ghost rows are dropped (the `i>0` filter).            */
int pa_mat_from_csc(pa_ctx* ctx, int dtype, int index_bytes,
                    int64_t nrows_lids, int64_t ncols_lids,
                    const void* colptr, const void* rowval, const void* nzval,
                    const pa_index* rows, const pa_index* cols,
                    pa_mat** out);
/* From the local SparseMatrixCSR{Bi} of one part (SparseUtils.jl:189-252;
 * PSparseMatrix(sparsecsr, I, J, V, rows, cols; ids), Interfaces.jl:
 * 2194-2215 with a CSR init): rowptr (nrows_lids+1) and colval hold
 * Bi-based indices (Bi = 0 or 1, index_bytes 4 or 8), nzval in storage
 * order.  Same SELL layout as pa_mat_from_csc; each owned row keeps its
 * owned-column entries in storage order, then its ghost-column entries in
 * storage order (the owned_owned then owned_ghost passes of
 * SparseUtils.jl:242-250), and mul! with α != 1 scales each product,
 * (v*x)*α, as SparseUtils.jl:247 does (a CSC parent scales x, :177).
 * pa_mat_set_values / pa_mat_get_values / pa_mat_xchg_create index the CSR
 * nonzeros.                                                             */
int pa_mat_from_csr(pa_ctx* ctx, int dtype, int index_bytes, int Bi,
                    int64_t nrows_lids, int64_t ncols_lids,
                    const void* rowptr, const void* colval, const void* nzval,
                    const pa_index* rows, const pa_index* cols,
                    pa_mat** out);
/* From COO triplets: PSparseMatrix(I, J, V, rows, cols; ids=:local)
 * (Interfaces.jl:2194-2244) → sparse(I, J, V, m, n, +) (SparseUtils.jl:
 * 80-94) on the device (stable radix sort, duplicates summed in input
 * order), then the same SELL layout as pa_mat_from_csc.  I, J: 1-based
 * local ids (index_bytes 4 or 8), ncoo entries each; an index out of range
 * is an error (BoundsError).  ids_global = 1 (ids=:global): I, J are Int64
 * global ids, mapped by to_lids! on the device through the gid tables of
 * rows and cols (pa_index_set_gids; an unknown gid is a KeyError).  *csc_nnz = nnz of the combined CSC; when
 * colptr_out (ncols_lids+1) / rowval_out (>= ncoo) are non-NULL the CSC
 * pattern is written there, 1-based, for host setup that needs it
 * (matrix_exchanger, Interfaces.jl:2300-2372).  The nonzeros' CSC order is
 * what pa_mat_set_values / pa_mat_get_values / pa_mat_xchg_create use.   */
int pa_mat_from_coo(pa_ctx* ctx, int dtype, int index_bytes, int ids_global,
                    int64_t nrows_lids, int64_t ncols_lids, int64_t ncoo,
                    const void* I, const void* J, const void* V,
                    const pa_index* rows, const pa_index* cols,
                    int64_t* csc_nnz, int64_t* colptr_out,
                    int64_t* rowval_out, pa_mat** out);
/* PSparseMatrix(sparsecsr, I, J, V, rows, cols; ids) with the compress on
 * the device: pa_mat_from_coo / pa_mat_from_dcoo with a SparseMatrixCSR{Bi}
 * parent — sparsecsr(Val(Bi), I, J, V, m, n, +) (SparseUtils.jl:193-208:
 * duplicates combined with + in input order, columns ascending in each
 * row), the matrix's nonzeros in CSR order and mul! with α applied to each
 * product (SparseUtils.jl:247), as pa_mat_from_csr.  *nnz = nonzeros;
 * rowptr_out (nrows_lids+1) / colval_out (>= ncoo), when non-NULL, receive
 * the CSR pattern in base Bi.  Needs ascending oid_to_lid / hid_to_lid in
 * cols (every PRange the reference builds).                              */
int pa_mat_from_coo_csr(pa_ctx* ctx, int dtype, int index_bytes, int ids_global, int Bi,
                        int64_t nrows_lids, int64_t ncols_lids, int64_t ncoo,
                        const void* I, const void* J, const void* V,
                        const pa_index* rows, const pa_index* cols, int64_t* nnz,
                        int64_t* rowptr_out, int64_t* colval_out, pa_mat** out);
int pa_mat_from_dcoo_csr(const pa_coo* coo, int ids_global, int Bi, int64_t nrows_lids,
                         int64_t ncols_lids, const pa_index* rows, const pa_index* cols,
                         int64_t* nnz, int64_t* rowptr_out, int64_t* colval_out,
                         pa_mat** out);
/* COO triplets of one part on the device: I, J global ids (Int64, 1-based),
 * V of dtype — the (I, J, V) of PSparseMatrix(I, J, V, rows, cols;
 * ids=:global), test_fem_sa.jl:60-131.                                  */
int pa_coo_create(pa_ctx* ctx, int dtype, int64_t n, const int64_t* I,
                  const int64_t* J, const void* V, pa_coo** out);
int pa_coo_destroy(pa_coo* coo);
int pa_coo_size(const pa_coo* coo, int64_t* n);
int pa_coo_download(const pa_coo* coo, int64_t* I, int64_t* J, void* V);
/* async_assemble!(I, J, V, rows) + wait (Interfaces.jl:2406-2492) over the
 * n parts of this process: each triplet whose row (a gid of rows, which
 * needs pa_index_set_gids) is owned by another part is sent to that owner —
 * segments in rows.exchanger.parts_rcv order, input order inside — and its
 * local value becomes zero (the entry stays); every part appends what it
 * receives in parts_snd order.  I and J stay global.  Parts of this process
 * exchange by device copies, other processes' parts by RCCL (counts first,
 * then I, J, V per segment).  A row gid that is not a local id of rows is
 * a KeyError (to_lids!, Interfaces.jl:2420).                              */
int pa_coo_assemble_all(int n, pa_coo* const coo[], const pa_index* const rows[],
                        pa_xchg* const rows_xchg[]);
/* async_exchange!(I, J, V, rows) + wait (Interfaces.jl:2494-2592) over the
 * n parts of this process, the mirror of pa_coo_assemble_all: each triplet
 * whose row (a gid of rows, which needs pa_index_set_gids) another part
 * holds as a ghost is copied to that part — segments in
 * rows.exchanger.parts_snd order, input order inside — and stays in the
 * local list unchanged.  A row that several neighbours hold goes to the
 * last of them in parts_snd order only (`lid_to_i[lid] = i` overwrites,
 * 2514-2520).  A triplet of a ghost row that is sent nowhere keeps its place
 * and its value becomes zero(Tv), an exact +0 (2529-2530).  Every part
 * appends what it receives in parts_rcv order.  I and J stay global.
 * Transport, preconditions and the KeyError of an unknown row gid as in
 * pa_coo_assemble_all; a neighbour that does not list the partner back is
 * an "exchanger mismatch" error.                                          */
int pa_coo_exchange_all(int n, pa_coo* const coo[], const pa_index* const rows[],
                        pa_xchg* const rows_xchg[]);
/* pa_mat_from_coo over a device COO (index_bytes 8): ids_global = 1 maps
 * I, J through rows' and cols' gid tables; the COO is left unchanged.    */
int pa_mat_from_dcoo(const pa_coo* coo, int ids_global, int64_t nrows_lids,
                     int64_t ncols_lids, const pa_index* rows,
                     const pa_index* cols, int64_t* csc_nnz,
                     int64_t* colptr_out, int64_t* rowval_out, pa_mat** out);
/* Replace the stored values keeping the pattern (same CSC nz order),
 * e.g. after fillstored!/re-assembly (Interfaces.jl:2127-2132).          */
int pa_mat_set_values(pa_mat* A, const void* nzval);
/* fillstored!(A, v) (Interfaces.jl:2127-2132): every stored value of the
 * part (ghost rows included) becomes the scalar *v of the matrix's dtype,
 * on the device, stream-ordered with the part's other work.              */
int pa_mat_fillstored(pa_mat* A, const void* v);
/* nonzeros(A) in CSC nz order, ghost rows included (the device keeps the
 * ghost rows' values beside the SELL slots for exchange!/assemble!(A)).  */
int pa_mat_get_values(const pa_mat* A, void* nzval);
/* ---- entry views of a PSparseMatrix --------------------------------------
 * The reads and writes of local_view / global_view over a matrix
 * (Interfaces.jl:2277-2298 over the LocalView / GlobalView getindex and
 * setindex! of 2004-2069), batched and on the device: the fixed-pattern
 * re-assembly loop `fillstored!(A, 0); a[gi, gj] += ke[i, j]; assemble!(A)`
 * without a host copy of nzval.
 * pa_mat_scatter: the n entries (I[k], J[k], V[k]) written into the stored
 * values of one part in input order, a[i, j] += v (op PA_SCATTER_ADD) or
 * a[i, j] = v (PA_SCATTER_SET: the last entry of an (i, j) in input order
 * stays).  The result equals the sequential loop bit for bit whatever the
 * duplicates: each entry's value index is looked up in the matrix's entry
 * table, the entries are sorted stably by it and each value's entries are
 * added onto it in input order by one thread, with plain adds (complex
 * values componentwise), no atomics — pa_vec_scatter's pass over the value
 * array.  Afterwards the copies of the values that the SpMV layouts keep
 * (side rows, triple SELL, uniform layout) are refreshed on the same stream,
 * so the next mul! / cg! / exchange!(A) / assemble!(A) / pa_mat_get_values
 * sees the new values.
 * pa_mat_gather: out[k] = a[I[k], J[k]].
 * Ids: PA_IDS_LOCAL: 1-based lids of rows / cols (index_bytes 4 or 8); one
 * outside 1..num_lids is an error (BoundsError).  PA_IDS_GLOBAL: 1-based
 * Int64 gids (index_bytes 8), looked up in the gid tables of rows and cols
 * (pa_index_set_gids); a gid that is no local id of its range is an error
 * (KeyError), except in pa_mat_gather with absent_zero = 1, where it reads
 * zero(T) (the LocalView read over another range, 2019-2026).  I and J are
 * never modified (the matrix views do not call to_lids!).  rows and cols
 * must be the index sets the matrix was built with.
 * Unstored entries: a valid (i, j) that the pattern does not store reads
 * zero(T), as SparseArrays' getindex does.  A write to it is an error: the
 * reference would insert the entry into the local CSC and change the
 * pattern; the device pattern is fixed (a deviation).
 * Every id of a call is checked before the first write: a failed call leaves
 * A unchanged.  n = 0 is legal.  on_device = 1: I, J and V (pa_mat_gather:
 * out) are device arrays on the part's device, otherwise host arrays
 * consumed before the call returns.  The work runs on the part's compute
 * stream, ordered with the part's other work.
 * The entry table — the sorted keys row_lid * num_lids(cols) + col_lid of
 * the stored entries (ghost rows and long rows included) with their value
 * indices, 16 B per stored entry — is built by a matrix's first view call
 * and kept; a matrix that never opens a view holds only the (row, col) lids
 * of its ghost-row nonzeros (8 B each).  Matrices from pa_mat_from_csc /
 * _csr / _coo[_csr] / _dcoo[_csr]; a pa_mat_stencil matrix has no nonzero
 * map and fails with a message, as pa_mat_set_values does.                 */
int pa_mat_scatter(pa_mat* A, pa_index* rows, pa_index* cols, int ids_kind,
                   int index_bytes, int op, int on_device, int64_t n,
                   const void* I, const void* J, const void* V);
int pa_mat_gather(const pa_mat* A, pa_index* rows, pa_index* cols, int ids_kind,
                  int index_bytes, int absent_zero, int on_device, int64_t n,
                  const void* I, const void* J, void* out);
/* The entry table of A: *entries = the stored entries it holds (the part's
 * owned-row nonzeros + its ghost-row nonzeros), 0 while no view call has
 * built it; *bytes = the device memory it takes.                          */
int pa_mat_entry_info(const pa_mat* A, int64_t* entries, int64_t* bytes);
/* findnz(A) / nziterator(A) of one part on the device (SparseUtils.jl:
 * 106-150, 254-300): the stored entries as a new device COO, the inverse of
 * pa_mat_from_dcoo and the first step of gather(A) (Interfaces.jl:2664-2704).
 * I and J are 1-based Int64: lids (PA_IDS_LOCAL), or gids through the
 * lid_to_gid of rows / cols (PA_IDS_GLOBAL: needs pa_index_set_gids).  V has
 * the matrix's dtype, one value per entry read from the main value array (the
 * copy every SpMV layout is refreshed from).  The COO owns its buffers
 * (pa_coo_destroy); A is unchanged.
 * which_rows: PA_NZ_OWNED_ROWS keeps the entries of the rows this part owns,
 * `rows.lid_to_part[i] == rows.part`, the filter of Interfaces.jl:2671-2687
 * (SELL slots, side rows and long rows alike); PA_NZ_ALL_ROWS adds the stored
 * ghost rows.
 * Order: the parent's nziterator order — ascending (col lid, row lid) for a
 * CSC parent, ascending (row lid, col lid) for a CSR parent, ghost rows in
 * their place.  Deviation: a pa_mat_from_csr parent whose rows are not
 * column-sorted gives every stored entry exactly once in ascending (row, col),
 * not in its storage order (the device keeps no copy of the parent's colval;
 * DESIGN.md 4.9).  Padding slots give nothing.
 * Route: the entry table's emit / compact / sort passes with the parent's
 * key, on pairs of the call's own — the matrix's entry table is neither read
 * nor built (pa_mat_entry_info is unchanged by the call).  All counts are
 * 64-bit.  The call runs on the part's compute stream and has completed on
 * it when it returns.  rows and cols must be the index sets the matrix was
 * built with; a pa_mat_stencil matrix has no nonzero map and fails with a
 * message, as the entry views do.  Bad arguments fail before anything is
 * allocated.                                                              */
#define PA_NZ_OWNED_ROWS 0
#define PA_NZ_ALL_ROWS 1
int pa_mat_findnz(pa_mat* A, pa_index* rows, pa_index* cols, int which_rows, int ids_kind,
                  pa_coo** out);
/* matrix_exchanger(values, rows, cols) (Interfaces.jl:2300-2372): the
 * Exchanger whose lids are CSC nz positions k (1-based, Int64 as Julia's
 * Table{Int}): k_rcv = nonzeros of ghost rows grouped by owner, k_snd = the
 * owner's nonzeros at the same (gi, gj).  Usable with pa_mat_exchange_all. */
int pa_mat_xchg_create(pa_mat* A, int32_t n_rcv, const int32_t* parts_rcv,
                       const int32_t* ptrs_rcv, const int64_t* k_rcv,
                       int32_t n_snd, const int32_t* parts_snd,
                       const int32_t* ptrs_snd, const int64_t* k_snd,
                       pa_xchg** out);
/* exchange!(A) (Interfaces.jl:2375-2381: op PA_REPLACE, reverse 0) and
 * assemble!(A) (2383-2404: op PA_ADD, reverse 1, zero_sent 1 — the ghost
 * rows' values are zeroed after sending) over nonzeros(A), n local parts.
 * Contributions to one nonzero are combined in the reference's order.     */
int pa_mat_exchange_all(int n, pa_mat* const A[], pa_xchg* const xg[],
                        int op, int reverse, int zero_sent);
int pa_mat_destroy(pa_mat* A);
/* nnz stored on device (padding included) and owned-row nnz. */
int pa_mat_info(const pa_mat* A, int64_t* nrows_owned, int64_t* nnz_owned,
                int64_t* slots, int64_t* nslices, int64_t* nslices_interior);
/* Column encoding chosen at build time: slices whose rows
 * mostly follow one offset pattern store no column ids ("pattern slices");
 * their other rows live in a side SELL.                                   */
int pa_mat_format_info(const pa_mat* A, int64_t* pattern_slices,
                       int64_t* regular_rows, int64_t* side_rows,
                       int64_t* side_slots);
/* delta16 slices (pa_tune "spmv_delta16", default on): int32-column slices
 * whose columns all fit 16-bit codes — an owned column as the row + a
 * signed 15-bit delta, a ghost column as the slice's smallest ghost column
 * + 15 bits — stream 2 B of column id per slot instead of 4.              */
int pa_mat_delta16_info(const pa_mat* A, int64_t* delta16_slices);
/* The triple SELL (pa_tune "spmv_tri16" 1, the default: Float64,
 * ComplexF32, ComplexF64 and Float32 with 2 rows per lane): the delta16 slices'
 * rows re-sliced — rows whose columns are consecutive triples (c, c+1, c+2)
 * first — so that most slices keep one 16-bit code per triple and read a
 * triple's x as one run.  Its slices and rows, and how many of them are
 * triple slices (tri_slices, their rows tri_rows).                       */
int pa_mat_triple_info(const pa_mat* A, int64_t* t_slices, int64_t* t_rows, int64_t* tri_slices,
                       int64_t* tri_rows);
/* The triple SELL's pair slices (pa_tune "spmv_tri_pack" bit 2, default on;
 * 2 rows per lane): each lane holds rows a and a + 1 whose columns differ
 * by one, entry for entry, and reads one code and one x run per triple for
 * both.  Its pair slices (counted in tri_slices too) and their rows.     */
int pa_mat_pair_info(const pa_mat* A, int64_t* pair_slices, int64_t* pair_rows);

/* device addresses of the matrix's main arrays, for placement diagnostics:
 * out[0..7] = values, int32 columns, slice offsets, slice lengths (pattern),
 * patterns, masks, side values, side columns (0 where absent)           */
int pa_mat_device_ptrs(const pa_mat* A, uint64_t out[8]);

/* Bytes one mul! streams from this matrix in its current encoding
 * (pa_tune("spmv_format")), as its kernels load them: values (padding
 * included), column ids (int32 slices, side rows, long rows) and slice
 * metadata (offsets, lengths, lists, patterns, masks, row maps).  The
 * bench's roofline adds x (read once), y and the halo to these.          */
int pa_mat_traffic(const pa_mat* A, int64_t* value_bytes, int64_t* index_bytes,
                   int64_t* meta_bytes);

/* Long rows (row-length histogram): rows with more than max(256, 8 × the
 * 90th-percentile row length) entries leave the SELL and run one wave per
 * row over their own CSR (in the reference's summation order unless
 * pa_tune("long_rows_exact", 0)).  Number of such rows and their nonzeros. */
int pa_mat_long_rows(const pa_mat* A, int64_t* n_long, int64_t* n_long_nnz);

/* ---- hot path -----------------------------------------------------------
 * mul!(c, a, b, α, β) (Interfaces.jl:2246-2275) for the n local parts:
 * starts the halo exchange of x (pack → P2P → unpack into x's ghost lids,
 * i.e. exchange!(b)), runs the interior slices meanwhile, then the slices
 * that read ghost values.  y_idx / x_idx are the partitions of c and b
 * (c.rows / b.rows); x_idx must have the matrix's column layout.
 * Asynchronous with respect to the host (stream-ordered per part).       */
int pa_spmv_all(int n, pa_mat* const A[], pa_vec* const y[],
                const pa_index* const y_idx[],
                pa_vec* const x[], const pa_index* const x_idx[],
                pa_xchg* const xg[], const void* alpha, const void* beta);

/* CG fusions (the caller of the hot path, IterativeSolvers.cg! at
 * test_fdm.jl:115 / test_fem_sa.jl:135):
 * pa_spmv_dot_all = mul!(c, A, u) followed by dot(u, c), the dot being
 * accumulated by the SpMV kernel over the owned rows it writes (u = x must
 * have contiguous owned lids); pa_cg_update_all = x .+= α.*u; r .-= α.*c
 * (all lids; the four vectors share one partition) and returns norm(r).
 * alpha is a Float64 (double) for real vectors, a ComplexF64 for complex
 * ones — IterativeSolvers' α = residual²/dot with a Float64 residual — and
 * each element is evaluated in that type and rounded once (PA_BCAST_*).
 * Reductions (dot, sum, norm) round each part's value to the element type
 * and add the parts in that type, as Julia's reduce over the parts' T
 * values does; norm's ^(1/2) is Float64.                                  */
int pa_spmv_dot_all(int n, pa_mat* const A[], pa_vec* const y[],
                    const pa_index* const y_idx[],
                    pa_vec* const x[], const pa_index* const x_idx[],
                    pa_xchg* const xg[], const void* alpha, const void* beta,
                    void* dot_result);
int pa_cg_update_all(int n, pa_vec* const x[], pa_vec* const r[],
                     const pa_vec* const u[], const pa_vec* const c[],
                     const pa_index* const idx[], const void* alpha,
                     double* rnorm);

/* ---- Jacobi-preconditioned CG ---------------------------
 * IterativeSolvers.cg!(x, A, b; Pl = Diagonal(diag(A))) over device
 * operations.  Float32 and Float64 only: with a complex element type all
 * three entries fail with a message before anything is touched (the scalar
 * recurrence's Complex/Complex divisions are not pinned by anything here).
 *
 * pa_mat_diag: d (num_lids(cols) elements of A's dtype) is set to zero(T)
 * everywhere, then for every owned row with a stored entry in its own column
 * d[col lid of that id] takes the stored value — diag(A) of the part's
 * owned block.  rows and cols are the matrix's index sets and must own the
 * same ids in the same order.  Stored ghost rows are skipped, an absent
 * diagonal stays +0.0, ghost lids stay +0.0 (the caller exchanges d).  The
 * (row, col) of a value is derived from what the matrix keeps for mul! —
 * the slice offsets and int32 columns of the SELL slots, the Float32
 * delta16 interleave of 4 rows per lane, the long rows' CSR, the columns'
 * oid_to_lid — one thread per owned row, plain stores (each row has at most
 * one such entry).  The entry table is neither used nor built
 * (pa_mat_entry_info is unchanged), nothing is copied to the host, and the
 * work is stream-ordered on the part's compute stream.  It reads the values
 * the owner stores, so for an FE matrix it belongs after assemble!(A).  A
 * matrix that does not keep that layout fails with a message, as
 * pa_mat_set_values does for one without a nonzero map (pa_mat_stencil
 * matrices keep the slots and their columns, so they have a diagonal here).
 *
 * pa_pcg_apply_all: c[i] = r[i] / d[i] over all lids — one IEEE division in
 * T per element, no reciprocal, what ldiv!(c, Diagonal(d), r) computes — and
 * *rho = dot(c, r) over the owned lids, accumulated in the same pass (rho: a
 * host scalar of the element type).  A zero in d gives Inf / NaN, as in
 * Julia.  c may be r.
 *
 * pa_pcg_update_all: the tail of one preconditioned iteration and the head
 * of the next in one pass over all lids: x .+= α.*u; r .-= α.*c;
 * c = r_new ./ d, and over the owned lids *rnorm = norm(r_new) and
 * *rho = dot(c_new, r_new).  alpha is a host scalar OF THE ELEMENT TYPE (the
 * preconditioned recurrence's α = ρ/dot(u, c) is a T, unlike
 * pa_cg_update_all's Float64 α): each element is evaluated in T, rounded at
 * every operation, no FMA.  The five vectors share one partition whose
 * owned lids are contiguous (0..noids-1: the reductions ride in the element
 * pass; anything else is an error, the caller checks).
 *
 * Reductions as the others': a Float64 accumulator, per-block partials
 * folded in block order, each part's value rounded to T, the parts added in
 * part order in T; norm's ^(1/2) is Float64.  pa_pcg_apply_all serves any
 * layout (ldiv! has no layout condition): with contiguous owned lids its dot
 * rides in the element pass, otherwise it runs as a reduction of its own
 * through oid_to_lid, same result.                                        */
int pa_mat_diag(const pa_mat* A, const pa_index* rows, const pa_index* cols, pa_vec* d);
int pa_pcg_apply_all(int n, pa_vec* const c[], const pa_vec* const r[], const pa_vec* const d[], const pa_index* const idx[], void* rho);
int pa_pcg_update_all(int n, pa_vec* const x[], pa_vec* const r[], const pa_vec* const u[], pa_vec* const c[], const pa_vec* const d[], const pa_index* const idx[], const void* alpha, double* rnorm, void* rho);

/* IterativeSolvers.cg!(x, A, b; reltol, abstol, maxiter) (v0.9, not
 * vendored; called at test_fdm.jl:115, test_fem_sa.jl:135, recurrence in
 * SURVEY.md §3.5) with the scalar recurrence on the device (SURVEY.md §8f
 * item 3): u, r, c are the caller's work vectors (CGStateVariables), all
 * five vectors on a.cols' partition with contiguous owned lids.  Setup as
 * cg_iterator!: u = 0, r = b - A*x, tolerance = max(reltol*norm(b), abstol).
 * Then per iteration β = res²/prev², u .= r .+ β.*u, mul!(c,A,u) with
 * dot(u,c) fused, α = res²/dot, x .+= α.*u, r .-= α.*c, res = norm(r) — the
 * same arithmetic as the host-driven loop over pa_spmv_dot_all /
 * pa_cg_update_all, bit for bit.  The host enqueues `batch` iterations
 * between reads of the device's done flag (iterations after convergence
 * are no-ops); every rank enqueues the same number, so RCCL calls match.
 * history (optional, maxiter doubles): the residual after each iteration. */
int pa_cg_solve_all(int n, pa_mat* const A[], pa_vec* const x[],
                    const pa_vec* const b[], pa_vec* const u[],
                    pa_vec* const r[], pa_vec* const c[],
                    const pa_index* const idx[], pa_xchg* const xg[],
                    double reltol, double abstol, int64_t maxiter, int batch,
                    int64_t* iterations, double* residual, double* history);

/* IterativeSolvers.cg!(x, A, b; Pl = Diagonal(d), reltol, abstol, maxiter)
 * (v0.9) with the scalar recurrence on the device: the
 * arguments and checks of pa_cg_solve_all, plus d, the diagonal on every lid
 * of the solve's range (pa_mat_diag followed by an exchange).  Float32 and
 * Float64 only.  Setup as cg_iterator!: u = 0, r = b - A*x, residual =
 * norm(r), tolerance = max(reltol*norm(b), abstol), ρ = one(T); unless the
 * solve is already done, c = r ./ d and ρ = dot(c, r) (pa_pcg_apply_all's
 * kernel).  Then per iteration β = ρ/ρ_prev, u .= c .+ β.*u, mul!(c, A, u)
 * with dot(u, c) fused, α = ρ/dot, x .+= α.*u, r .-= α.*c, c = r ./ d,
 * residual = norm(r), ρ_prev = ρ, ρ = dot(c, r) — ρ, β and α of the element
 * type, every operation rounded in it, the residual a Float64: the
 * arithmetic of the host-driven loop over pa_vec_axpby, pa_spmv_dot_all and
 * pa_pcg_update_all, bit for bit (x, history, iteration count).  The host
 * enqueues `batch` iterations between reads of the first part's done flag;
 * in the iterations of a batch that follow convergence (at most batch-1) the
 * kernels that write x, r, u and the state return at once, but mul!(c, A, u),
 * its dot and the gathers still run, so the work vector c holds A*u of the
 * last u on return.  Every rank enqueues the same number, so RCCL calls match.  Both modes of pa_cg_solve_all: every part of
 * one process, or one part per process over RCCL.  The u update always runs
 * as its own sweep (pa_tune "cg_fuse" does not apply).  It fails with a
 * message, before anything is touched, on a null argument or handle,
 * batch < 1, a complex element type, vectors of another size, element type
 * or context, and owned lids that are not contiguous.
 * history (optional, maxiter doubles): the residual after each iteration. */
int pa_pcg_solve_all(int n, pa_mat* const A[], pa_vec* const x[], const pa_vec* const b[],
                     const pa_vec* const d[], pa_vec* const u[], pa_vec* const r[], pa_vec* const c[],
                     const pa_index* const idx[], pa_xchg* const xg[], double reltol, double abstol,
                     int64_t maxiter, int batch, int64_t* iterations, double* residual, double* history);

/* The u-update variant choice of pa_cg_solve_all's auto mode (pa_tune
 * "cg_fuse" 2): the first timed batch runs the sweep, the second the fused
 * update; with one part per process (RCCL) every rank reduces the two
 * batch times with max over the ranks before choosing, so all ranks keep
 * the same variant.  pa_cg_variant_agree runs that decision on local_ms
 * (ms per iteration of the sweep and of the fused batch) with `fn` as the
 * all-reduce (max, in place on n floats; null: none), *choice = 1 fused,
 * 0 sweep, -1 no valid measurement.  pa_mat_cg_choice: the variant the
 * matrix remembers (-1: none yet).                                        */
typedef int (*pa_allreduce_max_fn)(float* v, int n, void* user);
int pa_cg_variant_agree(const float local_ms[2], pa_allreduce_max_fn fn, void* user, int* choice);
/* Whether the fused u update may run at all: only if every rank's part can
 * (no long rows, no triple SELL: their kernels gather x directly), or the
 * ranks would run different variants, whose halos carry different vectors
 * (ADVICE r05).  pa_cg_solve_all max-reduces "cannot fuse" over the ranks
 * (RCCL); this runs the same decision with fn as the all-reduce.  *agreed
 * = 1 when every rank's local_can_fuse is 1.                             */
int pa_cg_fuse_agree(int local_can_fuse, pa_allreduce_max_fn fn, void* user, int* agreed);
int pa_mat_cg_choice(const pa_mat* A, int* choice);

/* exchange!(combine, values, exchanger) (Interfaces.jl:846-889) for the n
 * local parts; reverse != 0 uses reverse(exchanger) (Interfaces.jl:796).
 * With reverse=1, op=PA_ADD and zero_ghosts=1 this is assemble!(v)
 * (Interfaces.jl:2084-2106).  Contributions to one lid are combined in the
 * receive-buffer order of the reference (bit-exact).                      */
int pa_exchange_all(int n, pa_vec* const v[], pa_xchg* const xg[],
                    const pa_index* const idx[], int op, int reverse,
                    int zero_ghosts);

/* ---- async exchange and completion handles -------------------------------
 * t = async_exchange!(…) / async_assemble!(…) (Interfaces.jl:349-401,
 * 2071-2106, 2375-2404): the same values in the same combine order as
 * pa_exchange_all / pa_mat_exchange_all, but all of part i's work (pack,
 * transport, unpack, zeroed ghosts / sent values) runs on part i's comm
 * stream, and done[i] completes behind the last of it.  The call returns at
 * once.  Part i's work starts after (a) everything enqueued so far on its
 * context, (b) after[i] when given (after: NULL, or n entries, each NULL or
 * an event of any context or device: the t0 of Interfaces.jl:369-373 without
 * a host wait), and (c) every earlier call that still uses the exchanger
 * buffers of part i or of its local peers.  Work enqueued later on the
 * compute stream does not wait for the call, except a later call on the same
 * exchanger, a context joined with pa_ctx_wait_event, and pa_ctx_sync.  From
 * the call until the wait or join the values belong to the call.  A failed
 * call leaves no handle in done.                                            */
int pa_exchange_all_async(int n, pa_vec* const v[], pa_xchg* const xg[],
                          const pa_index* const idx[], int op, int reverse,
                          int zero_ghosts, pa_event* const after[],
                          pa_event* done[]);
int pa_mat_exchange_all_async(int n, pa_mat* const A[], pa_xchg* const xg[],
                              int op, int reverse, int zero_sent,
                              pa_event* const after[], pa_event* done[]);
/* An event behind everything enqueued so far on ctx, on both its streams
 * (e.g. a mul! whose result an exchange takes as after[i]).               */
int pa_event_record(pa_ctx* ctx, pa_event** out);
/* *done = 1 once the event's work has finished, else 0; never blocks.     */
int pa_event_query(const pa_event* ev, int* done);
/* Blocks the host until this event's work has finished (nothing else).    */
int pa_event_wait(pa_event* ev);
/* Device-side join: what is enqueued on ctx's compute stream from now on
 * runs after the event; the host does not wait.                           */
int pa_ctx_wait_event(pa_ctx* ctx, const pa_event* ev);
/* Frees the handle; legal while its work is pending (the work goes on).   */
int pa_event_destroy(pa_event* ev);

/* ---- tables: exchange!(combine, values::AbstractPData{<:Table}, exchanger) --
 * One part's Table (Helpers.jl:63-94) on the device: row lid holds the data
 * entries ptrs[lid] .. ptrs[lid+1]-1, any number of them (the dof ids of a
 * cell, the unknowns of a node).  pa_table_create takes the nrows+1 1-based
 * Int32 ptrs from the host (ptrs_on_device = 0; consumed before the call
 * returns) or from the context's device (1; checked by a kernel): the first
 * must be 1 and they must not decrease, anything else is an error and
 * nothing is handed out.  The data (ptrs[nrows+1]-1 values of dtype, zero at
 * first) are reached through pa_table_data: a pa_vec view that the table
 * owns — pa_vec_upload / _download / _device_ptr / _fill work on it, and it
 * must not be destroyed (it goes with pa_table_destroy).  ptrs are immutable
 * after creation.  pa_table_info: the rows and the data entries.
 *
 * pa_table_exchange_all is the reference's Table exchange (Interfaces.jl:
 * 891-961) for the n local parts: the exchanger derived from xg[i] and the
 * table's ptrs (_table_exchanger / _table_lids_snd, 920-961: every lid
 * replaced by its row's data positions) drives the vector exchange over the
 * data.  The derivation runs on the device: the expanded
 * lid lists and the ordered combine plans are never built on or copied to the
 * host, which reads back one offset per neighbour.  A table keeps the derived
 * exchanger per base exchanger, so repeated exchanges of one table derive it
 * once.  op / reverse as pa_exchange_all (contributions to one data entry are
 * combined in the reference's receive-buffer order, bit-exact); zero_sent as
 * pa_mat_exchange_all: afterwards the data of the rows the transfer left
 * from are +0.0.  pa_table_exchange_all_async: the same with the event
 * semantics of pa_exchange_all_async (after, done); the derivation itself, on
 * a table's first call with an exchanger, completes before the call returns.
 *
 * Checks, all before any value moves (the tables are left as they were):
 * null handles, a table and an exchanger of different contexts, element
 * types that differ across parts and nrows smaller than the exchanger's
 * largest lid are errors raised before any allocation.  The expanded slots
 * of a side must fit Int32, as the reference's Table ptrs do.  For every
 * edge between two parts of the call the sender's and the receiver's
 * expanded segment lengths are compared; a difference is an error naming
 * both parts and both counts (the reference's @check on the segment sizes,
 * SequentialBackend.jl:187).  With a peer in another process the lengths are
 * the caller's contract, as the message sizes of MPI are in the reference:
 * both sides must hold rows of equal lengths for every slot pair; no sizes
 * are negotiated.                                                          */
int pa_table_create(pa_ctx* ctx, int dtype, int64_t nrows, const int32_t* ptrs,
                    int ptrs_on_device, pa_table** out);
int pa_table_destroy(pa_table* t);
int pa_table_data(pa_table* t, pa_vec** data);
int pa_table_info(const pa_table* t, int64_t* nrows, int64_t* ndata);
/* the nrows+1 1-based ptrs as the device holds them, into a host array */
int pa_table_ptrs(const pa_table* t, int32_t* ptrs);
int pa_table_exchange_all(int n, pa_table* const tables[], pa_xchg* const xg[],
                          int op, int reverse, int zero_sent);
int pa_table_exchange_all_async(int n, pa_table* const tables[], pa_xchg* const xg[],
                                int op, int reverse, int zero_sent,
                                pa_event* const after[], pa_event* done[]);

/* dot(a,b) (Interfaces.jl:1985-1992) → sum over parts, folded in part
 * order as reduce(+, …; init=0) (Interfaces.jl:221-238).  result: host
 * scalar of the vectors' dtype (complex: conj(a)·b).                      */
int pa_dot_all(int n, const pa_vec* const a[], const pa_index* const ia[],
               const pa_vec* const b[], const pa_index* const ib[],
               void* result);
/* norm(a, 2) (Interfaces.jl:1767-1772); result: host double (the
 * reference's `(…)^(1/p)` promotes Float32 partials to Float64).          */
int pa_norm2_all(int n, const pa_vec* const a[], const pa_index* const ia[],
                 void* result);
/* sum(a) = reduce(+, a; init=0) over owned values (Interfaces.jl:1973-1983) */
int pa_sum_all(int n, const pa_vec* const a[], const pa_index* const ia[],
               void* result);

/* ---- synthetic operators (benchmark driver, not a reference entry point) --
 * One Cartesian part box [box_lo, box_lo+box_n) of a gdims[0]×gdims[1]×
 * gdims[2] node grid (0-based coordinates, x fastest), built directly on the
 * device in the layout pa_mat_from_csc would produce for the CSC that the
 * drivers assemble: kind 7 = test_fdm.jl's FD Poisson operator (coeffs =
 * {diag, offdiag}), kind 27 = Q1-hex FE operator of test_fem_sa.jl's
 * pattern (coeffs = Ke, 8×8 row-major).  Owned lids are the box's nodes in
 * x-fastest order; shell_lid[(ez*(ny+2)+ey)*(nx+2)+ex] is the 0-based lid of
 * the node at box-local (ex-1,ey-1,ez-1) of the one-node shell (ghosts), or
 * -1; NULL when the part has no ghosts.  nlids_cols = noids + nhids.      */
int pa_mat_stencil(pa_ctx* ctx, int dtype, int kind, const int64_t gdims[3],
                   const int64_t box_lo[3], const int64_t box_n[3],
                   int64_t nlids_cols, const int32_t* shell_lid,
                   const double* coeffs, int ncoeffs, pa_mat** out);

/* ---- timing (PTimer analogue, PTimers.jl) -------------------------------
 * pa_ctx_set_timing(ctx, 1) starts recording the mul! calls of this context
 * with HIP events on the stream they run on (no synchronisation inside the
 * calls).  pa_ctx_kernel_times returns the means over the recorded calls of
 * the interior slices, the halo completion seen by the compute stream (wait
 * for the transport + unpack, after the interior slices) and the boundary
 * slices (+ long rows, fused-dot fold), and the number of calls; it clears
 * the record.  With the direct pull (parts sharing a stream pair,
 * halo_direct) no slice runs before the halo is complete: interior is 0,
 * halo is the pull kernel, boundary is every slice.
 * pa_ctx_last_kernel_ms: the interior and boundary means.                  */
int pa_ctx_set_timing(pa_ctx* ctx, int enable);
int pa_ctx_kernel_times(pa_ctx* ctx, float* interior_ms, float* halo_ms,
                        float* boundary_ms, int* count);
int pa_ctx_last_kernel_ms(pa_ctx* ctx, float* spmv_interior_ms,
                          float* spmv_boundary_ms);
/* Device time of a region on the compute stream: pa_ctx_span(ctx, 0) before
 * it, pa_ctx_span(ctx, 1) after it (event records, no synchronisation);
 * pa_ctx_span_ms waits for the end and returns the elapsed ms.  Parts whose
 * mul! runs grouped (shared stream pair) record their phase times on the
 * first part of the call only (pa_ctx_kernel_times: count 0 for the rest). */
int pa_ctx_span(pa_ctx* ctx, int stop);
int pa_ctx_span_ms(pa_ctx* ctx, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* PA_HIP_H */

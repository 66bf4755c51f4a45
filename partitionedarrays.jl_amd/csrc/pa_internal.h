// pa_internal.h — shared types of libpa_hip.so (host API + kernels).
//
// Element types follow Julia's arithmetic exactly (no FMA contraction: the
// whole library is compiled with -ffp-contract=off).  Complex products are
// Julia's `*(z::Complex, w::Complex)` = (zr*wr - zi*wi, zr*wi + zi*wr)
// (base/complex.jl), sums are componentwise.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pa_hip.h"

namespace pa {

struct alignas(8) c64 {
  float re, im;
};
struct alignas(16) c128 {
  double re, im;
};

__host__ __device__ inline c64 operator+(c64 a, c64 b) { return {a.re + b.re, a.im + b.im}; }
__host__ __device__ inline c64 operator-(c64 a, c64 b) { return {a.re - b.re, a.im - b.im}; }
__host__ __device__ inline c64 operator*(c64 a, c64 b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__host__ __device__ inline c128 operator+(c128 a, c128 b) { return {a.re + b.re, a.im + b.im}; }
__host__ __device__ inline c128 operator-(c128 a, c128 b) { return {a.re - b.re, a.im - b.im}; }
__host__ __device__ inline c128 operator*(c128 a, c128 b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

template <typename T> struct real_of { using type = T; };
template <> struct real_of<c64> { using type = float; };
template <> struct real_of<c128> { using type = double; };

// The wide type of Julia's mixed broadcasts with a Float64 / ComplexF64
// scalar (IterativeSolvers' α, β are Float64 even for Float32 vectors: norm
// of a PVector returns Float64, Interfaces.jl:1771): `r .+ β.*u` evaluates
// in W and rounds to T once on the store.
template <typename T> struct wide_of { using type = T; };
template <> struct wide_of<float> { using type = double; };
template <> struct wide_of<c64> { using type = c128; };
__host__ __device__ inline double widen(float v) { return (double)v; }
__host__ __device__ inline double widen(double v) { return v; }
__host__ __device__ inline c128 widen(c64 v) { return c128{(double)v.re, (double)v.im}; }
__host__ __device__ inline c128 widen(c128 v) { return v; }
template <typename T> __host__ __device__ inline T narrow(typename wide_of<T>::type v) { return (T)v; }
template <> __host__ __device__ inline c64 narrow<c64>(c128 v) { return c64{(float)v.re, (float)v.im}; }
template <> __host__ __device__ inline c128 narrow<c128>(c128 v) { return v; }
// Real * Complex is componentwise in Julia (base/complex.jl: x*real(z), x*imag(z))
__host__ __device__ inline double rscale(double a, double x) { return a * x; }
__host__ __device__ inline c128 rscale(double a, c128 z) { return c128{a * z.re, a * z.im}; }

template <typename T> __host__ __device__ inline T zero_of() { return T(0); }
template <> __host__ __device__ inline c64 zero_of<c64>() { return {0.f, 0.f}; }
template <> __host__ __device__ inline c128 zero_of<c128>() { return {0.0, 0.0}; }

// conj(a)*b, Julia's dot kernel for one element (LinearAlgebra: dot(x,y) = Σ dot(x_i,y_i))
__host__ __device__ inline float cdot(float a, float b) { return a * b; }
__host__ __device__ inline double cdot(double a, double b) { return a * b; }
__host__ __device__ inline c64 cdot(c64 a, c64 b) { return c64{a.re, -a.im} * b; }
__host__ __device__ inline c128 cdot(c128 a, c128 b) { return c128{a.re, -a.im} * b; }
// abs2
__host__ __device__ inline float abs2(float a) { return a * a; }
__host__ __device__ inline double abs2(double a) { return a * a; }
__host__ __device__ inline float abs2(c64 a) { return a.re * a.re + a.im * a.im; }
__host__ __device__ inline double abs2(c128 a) { return a.re * a.re + a.im * a.im; }

// ---- deterministic block reductions (shared by the .hip files) -----------
template <typename A>
__device__ inline A shfl_down64(A v, int d) {
  return __shfl_down(v, d, 64);
}
template <>
__device__ inline c128 shfl_down64<c128>(c128 v, int d) {
  return c128{__shfl_down(v.re, d, 64), __shfl_down(v.im, d, 64)};
}

// 256-thread block sum in a fixed order (wave tree, then waves 0..3); the
// result is valid on thread 0
template <typename A>
__device__ inline A block_reduce(A v) {
  __shared__ A sm[4];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + shfl_down64(v, d);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  A r = zero_of<A>();
  if (threadIdx.x == 0) {
    r = sm[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = r + sm[i];
  }
  return r;
}

// In-launch hand-off of one value per block (cdna_hip_programming.md §6
// Guideline 16, R1 with a ticket counter): lane 0 stores its value
// write-through (sc1), drains, then takes a ticket; the block whose ticket
// is the last one reads every value with sc1 loads.  The ticket is zeroed at
// allocation and reset by the last block, so it is 0 between launches.
typedef __attribute__((address_space(1))) unsigned long long pa_gu64;
typedef __attribute__((address_space(1))) unsigned int pa_gu32;

__device__ inline void st_wt(double* p, double v) {
  __hip_atomic_store((pa_gu64*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st_wt(c128* p, c128 v) {
  st_wt(reinterpret_cast<double*>(p), v.re);
  st_wt(reinterpret_cast<double*>(p) + 1, v.im);
}
__device__ inline double ld_wt(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((pa_gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ inline c128 ld_wt(const c128* p) {
  const double* q = reinterpret_cast<const double*>(p);
  return c128{ld_wt(q), ld_wt(q + 1)};
}

// every thread of the block gets: did this block arrive last?
template <typename A>
__device__ inline bool publish_arrive(A* slots, A v, unsigned* ticket) {
  __shared__ int last;
  if (threadIdx.x == 0) {
    st_wt(&slots[blockIdx.x], v);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add((pa_gu32*)ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = t == gridDim.x - 1;
    if (last) __hip_atomic_store((pa_gu32*)ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return last != 0;
}

struct NoTail {
  __device__ void operator()(const void*) const {}
};

constexpr int kFoldBlocks = 256;  // first-level blocks of a long fold (scratch: kFoldBlocks accumulators)

// Fold nb partials into out[0] in ONE launch, in the order of the two-level
// fold it replaces (k_fold_chunks + k_reduce_final): with g > 1 blocks,
// block b sums chunk [b*chunk, (b+1)*chunk) and hands it over; the last
// block sums the g chunk sums in block order.  tail(out) then runs on
// thread 0 of the finishing block (e.g. the CG scalar update).
template <typename A, typename Tail>
__global__ __launch_bounds__(256) void k_fold(int nb, int chunk, const A* __restrict__ in, A* scratch,
                                              A* __restrict__ out, unsigned* ticket, Tail tail) {
  const bool one = gridDim.x == 1;
  const int lo = one ? 0 : (int)blockIdx.x * chunk;
  const int hi = one ? nb : min(nb, lo + chunk);
  A s = zero_of<A>();
  for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) s = s + in[i];
  A r = block_reduce(s);
  if (!one) {
    if (!publish_arrive(scratch, r, ticket)) return;
    A s2 = zero_of<A>();
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) s2 = s2 + ld_wt(&scratch[i]);
    r = block_reduce(s2);
  }
  if (threadIdx.x == 0) {
    out[0] = r;
    tail(out);
  }
}

template <typename A, typename Tail>
inline void fold_launch(int nb, const A* in, A* scratch, A* out, unsigned* ticket, Tail tail, hipStream_t st) {
  int g = 1, chunk = nb;
  if (nb > 2 * kFoldBlocks && scratch) {  // one block over 10^5 partials is ~150 us
    chunk = (nb + kFoldBlocks - 1) / kFoldBlocks;
    g = (nb + chunk - 1) / chunk;
  }
  hipLaunchKernelGGL((k_fold<A, Tail>), dim3(g), dim3(256), 0, st, nb, chunk, in, scratch, out, ticket, tail);
}

inline size_t dtype_size(int dt) {
  switch (dt) {
    case PA_F32: return 4;
    case PA_F64: return 8;
    case PA_C64: return 8;
    case PA_C128: return 16;
  }
  return 0;
}

// Rows per lane of the SELL layout so that one lane's value load is 16 B
// (Float32: pa_tune "f32_rows" 2 gives 8 B loads in 128-row slices, the
// Float64 geometry, so its delta16 rows can take the triple SELL).
int f32_rows_knob();
// finalize_pattern's answer for a Float32 matrix built with 4 rows per lane
// under f32_rows 0 (auto) that is better off with 2: the caller rebuilds it
constexpr int kPreferR2 = 2;
inline int sell_rows_per_lane(int dt) {
  switch (dt) {
    case PA_F32: return f32_rows_knob();
    case PA_F64: return 2;
    case PA_C64: return 2;
    case PA_C128: return 1;
  }
  return 1;
}

void set_error(const std::string& msg);

// Device-resident scalars of the device-driven CG (pa_cg_solve_all): the
// IterativeSolvers 0.9 recurrence state, one copy per part (every part
// folds the same gathered partials in part order, so all copies agree).
struct CGState {
  double res;        // it.residual = norm(r)
  double prev;       // it.prev_residual
  double tol;        // max(reltol*norm(b), abstol)
  int64_t it;        // iterations done
  int64_t maxiter;
  int32_t done;      // it >= maxiter || res <= tol
  int32_t pad;
  c128 alpha;        // α in the wide type: Float64 (.re) for real T, ComplexF64 for complex T
  int64_t xit;       // iterations whose x .+= α.*u is applied (deferred into the next u update)
};

// Device-resident scalars of the device-driven Jacobi-preconditioned CG
// (pa_pcg_solve_all), one copy per part as above.  Unlike
// CGState's, the recurrence's scalars are of the element type T: rho,
// rho_prev and alpha hold T values (a Float32 widened exactly) and the
// kernels convert them back before every operation, which then runs in T.
struct PCGState {
  double res;        // norm(r), Float64
  double tol;        // max(reltol*norm(b), abstol)
  int64_t it;        // iterations done
  int64_t maxiter;
  int32_t done;      // it >= maxiter || res <= tol
  int32_t pad;
  double rho;        // ρ = dot(Pl \ r, r) of the current r
  double rho_prev;   // the ρ of the iteration before (one(T) before the first)
  double alpha;      // α = ρ / dot(u, A*u)
};

// Grouped launches (parts of one process sharing a stream pair): one launch
// per phase covers up to PA_GROUP_MAX parts (kernel-argument tables).
constexpr int PA_GROUP_MAX = 8;
constexpr int32_t kTriSlice = 1 << 30;  // TripleSell::len: a triple slice
constexpr int32_t kTriPair = 1 << 29;   // TripleSell::len: a pair slice (lane l: rows a_l, a_l + 1; build_triple_sell)
constexpr int32_t kTriLen = kTriPair - 1;  // TripleSell::len: the entries per row
// The slice kinds of a mul!: which of a pa_mat's structures
// and column encodings a launch entry runs.  kind_desc (pa_spmv.hip) holds
// what each kind reads; slice_list (pa_api.cpp) a matrix's entries per phase.
enum SliceKind : int {
  kPattern = 0,  // pattern slices of the main structure
  kInt32 = 1,    // int32-column slices of the main structure
  kSide = 2,     // side SELL
  kDelta16 = 4,  // delta16 slices of the main structure
  kTriple = 5,   // triple SELL
};
// the kernels' PK / PAT template parameter: the column encoding of a wave's slice
constexpr int kPkInt32 = 0, kPkPattern = 1, kPkDelta16 = 3, kPkTriple = 4;

struct SpmvPart {
  int64_t nwork;          // slices of this part in the launch
  const int32_t* list;    // slice ids (null: 0..nwork-1)
  const pa_mat* A;
  const void* x;
  void* y;
  const int32_t* ymap;
  void* dotp;
  // the device CG's fused u update (pa_cg_solve_all; null cg: a plain SpMV):
  // x is r, the SpMV multiplies u_new = r .+ β.*xu, writes u_new of the owned
  // rows to un and applies the deferred x .+= α.*xu to xacc
  const void* xu = nullptr;
  void* un = nullptr;
  void* xacc = nullptr;
  const CGState* cg = nullptr;
  // a side-row entry (kSide) trailing the pattern entries of one grouped
  // kPattern launch (spmv_grouped's side tail)
  bool side = false;
};

struct PackGroup {
  int np;
  int64_t n[PA_GROUP_MAX];
  const int32_t* lids[PA_GROUP_MAX];
  const void* v[PA_GROUP_MAX];
  void* buf[PA_GROUP_MAX];
};
struct PullGroup {
  int np;
  int64_t n[PA_GROUP_MAX];
  const int32_t* lids[PA_GROUP_MAX];
  const int32_t* bid[PA_GROUP_MAX];
  const int64_t* elem[PA_GROUP_MAX];
  const void* const* bases[PA_GROUP_MAX];
  void* v[PA_GROUP_MAX];
};

// One part's share of a broadcast expression (pa_vec_eval /
// pa_reduce_expr_all), passed to the kernels of pa_expr.hip by value: the
// program and the operand numbers are wave-uniform, so the interpreter's
// branches are scalar branches.
struct ExprArgs {
  pa_expr prog;
  int nvec;
  const void* v[PA_EXPR_MAX_VECS];
  const int32_t* map[PA_EXPR_MAX_VECS];  // element i of operand k is v[k][map[k][i]] (null: i)
  c128 scal[PA_EXPR_MAX_SCALARS];        // widened (exactly); a real scalar has im = 0
};
// y[ymap[i]] = prog(i) for i < n; fast: every map is null (16 B per lane and operand)
void launch_expr_store(int dtype, int64_t n, const ExprArgs& a, void* y, const int32_t* ymap, bool fast,
                       hipStream_t st);
// kind PA_REDUCE_*: the part's value (double / c128 accumulator) into result[0]
void launch_expr_reduce(int dtype, int kind, int64_t n, const ExprArgs& a, bool fast, void* partials,
                        void* result, unsigned* ticket, hipStream_t st);

// Cartesian part box of a synthetic stencil operator (pa_mat_stencil).
struct StencilGeom {
  int64_t N[3];   // global nodes per dim
  int64_t lo[3];  // box origin (0-based global coords)
  int64_t n[3];   // box extent
  int kind;       // 7 (test_fdm.jl FD) or 27 (Q1 FE, test_fem_sa.jl pattern)
};

}  // namespace pa

// ---------------------------------------------------------------------------
// Opaque handle definitions.
struct pa_ctx {
  // parts of one process on the same device may share one stream pair
  // (pa_ctx_create_shared): their work then forms one in-order chain
  struct StreamRefs { int n = 1; };
  StreamRefs* stream_refs = nullptr;
  int device = 0;
  int part = 1;    // 1-based
  int nparts = 1;
  hipStream_t s_main = nullptr;   // compute stream
  hipStream_t s_comm = nullptr;   // halo transport stream (high priority)
  void* comm = nullptr;           // ncclComm_t (null: no remote transport)
  bool halo_rccl = false;         // pa_comm_init_all: halo segments between parts of this process over RCCL too
  // the communicator is destroyed with the last part using it; parts of one
  // device share their device's rank (pa_comm_init_all), so the peer of a
  // halo segment from/to part q is rank_of_part[q-1] (null: rank = q-1)
  std::shared_ptr<void> comm_owner;
  std::shared_ptr<const std::vector<int>> rank_of_part;
  int peer_rank(int q) const { return rank_of_part ? (*rank_of_part)[q - 1] : q - 1; }
  int64_t rccl_bytes_sent = 0, rccl_bytes_recv = 0;  // halo bytes this part posted to RCCL (pa_comm_stats)
  // reduction scratch
  void* d_partials = nullptr;     // per-block partials (max 16 B each)
  void* d_fold = nullptr;         // 256*16 B first-level fold of long partial lists
  void* d_result = nullptr;       // 16 B final per-part value
  void* d_gather = nullptr;       // nparts*16 B gathered partials (RCCL mode)
  unsigned* d_ticket = nullptr;   // arrival counter of the one-launch folds (0 between launches)
  void* h_pinned = nullptr;       // pinned host staging (>= nparts*16 B)
  // timing (pa_ctx_set_timing): four events per recorded mul! — before the
  // interior slices, after them, after the halo wait (+unpack), after the
  // boundary slices — read back only by pa_ctx_kernel_times (no sync per call)
  bool timing = false;
  std::vector<hipEvent_t> tev;
  int tn = 0;                     // mul! calls recorded since timing was enabled
  hipEvent_t span_ev[2] = {nullptr, nullptr};  // pa_ctx_span: start / end of a region
  // events for the exchange pipeline
  hipEvent_t ev_packed = nullptr;
  hipEvent_t ev_recvd = nullptr;
  // the pack barrier of stream-pair mul! calls this part leads (spmv_impl's
  // barrier issue): recorded on its s_comm once every part of the call packed
  hipEvent_t ev_barrier = nullptr;
  // device arrays of the x pointers of grouped mul! calls led by this part
  // (the direct pull's bases), most recent first
  std::vector<std::pair<std::vector<void*>, void**>> bases_cache;
  // device copies of the merged-launch tables of calls led by this part
  std::vector<std::pair<std::vector<char>, void*>> merged_cache;
  // pa_ctx_tune: this context's knob values over the process defaults,
  // applied to the calls it leads (TuneScope)
  static constexpr int kMaxKnobs = 24;
  bool has_over[kMaxKnobs] = {};
  int64_t over[kMaxKnobs] = {};
};

// Completion of one call's work for one part (pa_exchange_all_async: [0] the
// compute stream's work before the call, [1] the end of the call's work on
// the comm stream; pa_event_record: [0] the compute stream, [1] the comm
// stream).  The handle owns its events (no timing) on its device.
struct pa_event {
  int device = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

// The tuning knobs of one call (performance only, results unchanged; the
// table with their meaning is kKnobs in pa_api.cpp).  A call resolves them
// once — the process defaults (pa_tune) under its first part's context
// overrides (pa_ctx_tune) — into its own Knobs, which the launchers and the
// IssuePool jobs of that call read through pa::knobs(): no process-global
// knob is written while a call runs, so concurrent calls from several host
// threads each see their own context's values.
namespace pa {
struct Knobs {
  int spmv_flags;        // SPMV_* bits of pa_spmv.hip
  int long_exact;
  int halo_pull;
  int spmv_delta16;
  int spmv_merge;
  int64_t spmv_merge_max;
  int cg_fuse;
  int halo_direct;
  int halo_transport;
  int spmv_group;
  int spmv_format;
  int pattern_min_pct;
  int issue_threads;
  int fault_inject;      // tests only: the IssuePool jobs issue an invalid launch
  int spmv_xcd_chunk;    // XCD-chunked block order of the SpMV launches (pa_spmv.hip xcd_block), 0 off, -1 auto
  int spmv_tri16;        // delta16 slices re-sliced into the triple SELL (pa_mat::d_t_*): 0 never, 1 R <= 2
  int halo_barrier;      // stream-pair mul!: one pack barrier + double-buffered sends (spmv_impl)
  int tri_order;         // triple SELL row order: 0 triple rows first, 1 the other rows first (build_triple_sell)
  int side_tail;         // per-kind launches: the side rows as the trailing waves of the pattern launch
  int f32_rows;          // Float32 SELL rows per lane (matrices built afterwards): 4 (16 B packs), 2 (8 B), 0 auto
  int tri_pack;          // triple SELL: bit 2 pair slices, bit 0 their Float32 per-triple value packs
  int spmv_uniform;      // Float64 short pattern rows: the uniform layout (build_uniform)
  int scatter_wide;      // ordered vector scatter: 64-bit sort keys and payloads even when 32 bits fit
};
// the knobs of the call running on this thread (outside a call: a snapshot
// of the process defaults)
const Knobs& knobs();
// this thread runs work of a call whose knobs are *k (IssuePool workers)
struct KnobBind {
  explicit KnobBind(const Knobs* k);
  ~KnobBind();
  const Knobs* prev;
};
}  // namespace pa

// the knobs of a call's (first part's) context for the call's duration
struct TuneScope {
  explicit TuneScope(const pa_ctx* c);
  ~TuneScope();
  TuneScope(const TuneScope&) = delete;
  TuneScope& operator=(const TuneScope&) = delete;
  pa::Knobs k;
  const pa::Knobs* prev;
};

namespace pa {
// A device array and its owner (move-only).  It converts to its pointer, so
// launches and copies take it as they would the raw pointer.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) adopt(o.p), o.p = nullptr;
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() { adopt(nullptr); }
  void adopt(T* q) {  // takes over an allocation of the HIP allocator
    if (p) (void)hipFree(p);
    p = q;
  }
  hipError_t alloc(size_t n) {  // n elements (bytes for DevBuf<void>), uninitialised
    reset();
    return hipMalloc((void**)&p, n * sizeof(std::conditional_t<std::is_void<T>::value, char, T>));
  }
  template <typename U>
  hipError_t upload(const std::vector<U>& h) {  // an empty vector leaves the buffer null
    static_assert(std::is_same<U, T>::value, "element type");
    reset();
    if (h.empty()) return hipSuccess;
    const hipError_t e = alloc(h.size());
    return e != hipSuccess ? e : hipMemcpy(p, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice);
  }
  operator T*() const { return p; }
  template <typename U>
  explicit operator U*() const { return (U*)p; }
};
// n elements of a device array into h, on st (the caller synchronises)
template <typename T>
inline hipError_t download(std::vector<T>& h, const T* d, size_t n, hipStream_t st) {
  h.resize(n);
  return hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, st);
}
}  // namespace pa

struct pa_index {
  pa_ctx* ctx = nullptr;
  uint64_t id = 0;           // unique per index set of the process (cache keys)
  int64_t nlids = 0, noids = 0, nhids = 0;
  bool own_contig = true;    // oid_to_lid == 0..noids-1 (0-based)
  bool ghost_contig = true;  // hid_to_lid == noids..nlids-1
  pa::DevBuf<int32_t> d_oid_to_lid;  // 0-based, null when own_contig
  pa::DevBuf<int32_t> d_hid_to_lid;  // 0-based, null when ghost_contig
  std::vector<int32_t> h_oid_to_lid;  // 0-based host copies
  std::vector<int32_t> h_hid_to_lid;
  std::vector<int32_t> h_lid_to_ohid;  // reference's lid_to_ohid (1-based ±)
  // gid → lid table (pa_index_set_gids): gids sorted ascending, their lids
  pa::DevBuf<uint64_t> d_sgid;
  pa::DevBuf<int64_t> d_slid;
  pa::DevBuf<int64_t> d_lid_to_gid;  // nlids 1-based gids (to_gids!, pa_mat_findnz with global ids)
  bool has_gids = false;
};

// Ordered combine plan: for each distinct target lid, the buffer positions
// that land on it, ascending (= the reference's unpack loop order).
struct pa_combine_plan {
  int64_t ntargets = 0;
  bool unique = true;                // every lid at most once → plain scatter
  pa::DevBuf<int32_t> d_target;      // distinct target lids (0-based)
  pa::DevBuf<int32_t> d_ptr;         // ntargets+1
  pa::DevBuf<int32_t> d_pos;         // buffer positions
};

// Pull table of one exchange direction (parts of one process): receive slot
// p of this part reads bases[bid[p]][elem[p]] — a sender's send buffer, or
// this part's own receive buffer for segments that came over RCCL.
struct pa_pull {
  bool built = false;
  bool ok = false;                   // false: peers not reachable, use staging copies
  std::vector<const void*> key;      // the local senders (exchanger ids) and buffers the table was built for
  pa::DevBuf<int32_t> d_bid;
  pa::DevBuf<int64_t> d_elem;
  pa::DevBuf<void*> d_bases;
};

namespace pa {
// One neighbour list of an exchanger
struct XchgSide {
  std::vector<int32_t> parts;   // 1-based
  std::vector<int64_t> ptrs;    // 0-based offsets, size n+1
  int64_t n = 0;                // slots
  DevBuf<int32_t> lids;         // 0-based
  DevBuf<void> buf;             // 16 B per slot
  pa_combine_plan plan;         // unpack targets = this side's lids
};
// COO triplets on the device: global row/column ids (Int64) and values
struct CooList {
  DevBuf<int64_t> I, J;
  DevBuf<void> V;
  int64_t n = 0;
};
// The ordered scatter of n pairs (id, V) into one part's values and its
// gather twin (pa_coo.hip; pa_vec_scatter / pa_vec_gather).  I, V, out are
// device arrays; global: I holds Int64 gids looked up in (sgid, slid).  Both
// return 1 when an id has no lid (the scatter then wrote nothing), -1 on a
// HIP error, and have completed on st when they return.
int vec_scatter(int dtype, int64_t nl, void* v, bool global, int index_bytes, bool set, bool zero_first, bool wide,
                int64_t n, void* I, const void* V, const uint64_t* sgid, const int64_t* slid, hipStream_t st);
int vec_gather(int dtype, int64_t nl, const void* v, bool global, int index_bytes, bool absent_zero, int64_t n,
               const void* I, void* out, const uint64_t* sgid, const int64_t* slid, hipStream_t st);
}  // namespace pa

struct pa_xchg {
  pa_ctx* ctx = nullptr;
  uint64_t id = 0;                             // unique per exchanger of the process (cache keys)
  pa_pull pull[2];                             // [0] forward, [1] reverse
  // direct pull of mul! over parts sharing one stream pair (spmv_grouped):
  // receive slot p reads x of the call's part bid[p] at lid elem[p] (the
  // sender's snd.lids entry), no pack, no send buffer, no cross-stream event
  pa_pull direct;
  std::vector<int32_t> h_lids_snd;             // 0-based host copies (vector exchangers)
  std::vector<int32_t> h_lids_rcv;
  // a lid of lids_snd is also in lids_rcv (legal: every part packs before any
  // unpacks, the old value travels): the direct pull, which reads the
  // senders' x while it writes the receivers', is not taken (build_direct)
  bool snd_in_rcv = false;
  // lids_rcv names an owned lid of the index set with id own_key (0: not
  // looked at yet): the halo then also writes what the interior slices read,
  // and mul! runs them after it (halo_writes_owned)
  uint64_t own_key = 0;
  bool rcv_owned = false;
  // forward (dir 0, exchange!): snd's slots travel to the neighbours' rcv;
  // reverse (dir 1, assemble!): rcv's slots travel to the neighbours' snd
  pa::XchgSide rcv, snd;
  // the side a transfer in direction dir lands on / leaves from
  pa::XchgSide& into(int dir) { return dir ? snd : rcv; }
  const pa::XchgSide& into(int dir) const { return dir ? snd : rcv; }
  pa::XchgSide& from(int dir) { return into(1 - dir); }
  const pa::XchgSide& from(int dir) const { return into(1 - dir); }
  int64_t max_lid = -1;                        // 0-based, over both lists
  // the barrier issue of stream-pair mul! (spmv_impl): a second forward send
  // buffer, used every other call, and the pull table against the senders'
  // second buffers; the last barrier call these exchangers took part in
  // (key of its exchanger set, its sequence number, the buffer it packed)
  pa::DevBuf<void> buf_snd2;
  pa_pull pull_alt;
  uint64_t fast_key = 0, fast_seq = 0;
  int fast_parity = 0;
};

constexpr size_t kVecPad = 64;  // bytes before and after a vector's values (pa_vec_create)

// COO triplets of one part on the device, the input of
// async_assemble!(I, J, V, rows) and PSparseMatrix(I, J, V, …)
struct pa_coo {
  pa_ctx* ctx = nullptr;
  int dtype = PA_F64;
  pa::CooList l;
};

struct pa_vec {
  pa_ctx* ctx = nullptr;
  int dtype = PA_F64;
  int64_t n = 0;
  void* d = nullptr;        // the values (base + kVecPad)
  pa::DevBuf<void> base;    // the allocation (null for views)
};

// One part's Table on the device (Helpers.jl:63-94): the row offsets and the
// data as a vector, and the derived exchangers of the exchange!(Table) calls
// it took part in (pa_table.hip), one per base exchanger id.  ptrs never
// change after creation, so a derived exchanger stays valid for the table's
// lifetime; it owns its lid lists, buffers and combine plans like any pa_xchg.
struct pa_table {
  pa_ctx* ctx = nullptr;
  int dtype = PA_F64;
  int64_t nrows = 0, ndata = 0;
  pa::DevBuf<int32_t> t;     // nrows + 1 offsets, 0-based
  pa_vec* data = nullptr;    // ndata values (pa_table_data hands out this view)
  std::vector<std::pair<uint64_t, std::unique_ptr<pa_xchg>>> plans;
};

namespace pa {
// pa_table.hip
hipError_t table_ptrs(int64_t nrows, const int32_t* d_ptrs1, int32_t* t, int* bad, int64_t* ndata, hipStream_t st);
int table_expand_side(const XchgSide& in, const int32_t* t, XchgSide* out, int64_t* total, hipStream_t st,
                      hipError_t* err);
}  // namespace pa

// int32 words of a pattern slice's descriptor (dedup_patterns, SPMV_DESC):
// 4 header words + the slice's H/64 64-bit mask words, a power of two
constexpr int desc_words(int R) { return R <= 2 ? 8 : 16; }

namespace pa {
// The kind of a slice of the main structure as the build records it
// (pa_mat::h_kind, pa_mat::d_kind; k_pattern_detect, k_delta16 and k_u_fill
// write and read the numbers).  The device copy holds kBkInt32, kBkPattern
// and kBkDelta16 only: a delta16 slice whose rows moved to the triple SELL
// stays kBkDelta16 there (spmv_format 0 still runs it, and reads its
// interleaved Float32 layout from that value) and is kBkMoved on the host.
enum BuildKind : int32_t { kBkInt32 = 0, kBkPattern = 1, kBkDelta16 = 3, kBkMoved = 5 };

// One sliced-ELL structure: slice s holds rows [s*H, (s+1)*H) of the
// structure in len[s] entries per row at slot offset off[s].
struct Sell {
  int64_t nrows = 0, nslices = 0;
  int64_t slots = 0;          // incl. padding
  int maxlen = INT32_MAX;     // longest row (SH kernels when <= 8)
  DevBuf<int64_t> off;        // nslices
  DevBuf<int32_t> len;        // nslices (entries per row, max over the slice)
  DevBuf<int32_t> col;        // slots: x lid (0-based) or -1 padding
  DevBuf<uint16_t> col16;     // slots: 16-bit codes (delta16 slices, triple SELL)
  DevBuf<int32_t> gbase;      // per slice: smallest ghost column (base of the ghost codes)
  DevBuf<void> val;           // slots (the main structure: then the ghost-row and long-row values)
  DevBuf<int32_t> rowmap;     // structure row -> oid (null: the identity)
  DevBuf<int32_t> rowlen;     // structure row -> its entries
};
// The slices of one kind by phase: without ghost reads (before the halo) and with
struct SliceSet {
  int64_t n_int = 0, n_bnd = 0;
  DevBuf<int32_t> d_int, d_bnd;
};
// Triple SELL (pa_tune "spmv_tri16"): the rows of the
// delta16 slices, re-sliced by class — rows whose column list is
// consecutive triples (c, c+1, c+2) first, then the other rows, each class
// by length (descending) and oid — with a row map.  A "tri" slice (every
// row regular, length % 3 == 0) keeps one 16-bit code per triple and its
// lane reads a triple's x as one run; the other slices keep one code per
// entry.  Rows of a slice are interleaved (row i at lane i % 64, position
// i / 64).  Values are copies of the main slots (refreshed with the side
// SELL); the main delta16 slices are not launched then (kBkMoved).
// len: entries per row, bit 30: tri slice (kTriSlice), bit 29: pair slice;
// col16: tri slices one code per triple (slot groups 0..len/3-1);
// val: lane-major packs of R like the main SELL (pack: tri slices per triple)
struct TripleSell : Sell {
  SliceSet list;
  DevBuf<int64_t> src;        // structure row -> its main-layout slot of entry 0 (entry k: + k*64*R)
  DevBuf<int32_t> desc;       // per slice {offset / H, len, gbase, 0} (SPMV_DESC)
  int pack = 0;               // slices of 2 rows per lane (spmv_tri_pack): bit 2 pair slices; bit 0 (Float32)
                              // a pair slice's triple t as {entries 0,1 x R rows} 16 B + {entry 2} 8 B per lane
  int64_t tri_slices = 0, tri_rows = 0, code_slots = 0;
  int64_t pair_slices = 0, pair_rows = 0;  // pair slices and the rows they hold
  std::vector<int32_t> h_len;  // host copy for pa_mat_traffic
};
// the uniform layout of short pattern rows (build_uniform): K = |U| <= 7
// entries per row at slice * H * K, U's offsets, pattern id -> U position
struct UniformRows {
  DevBuf<void> val;
  DevBuf<int32_t> emap;
  int K = 0;
  int32_t pat[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
}  // namespace pa

struct pa_mat {
  pa_ctx* ctx = nullptr;
  int dtype = PA_F64;
  int cg_fuse_choice = -1;   // device CG with cg_fuse 2 (auto): the faster u-update variant measured on this matrix
  int R = 2;                 // rows per lane
  int H = 128;               // rows per slice = 64*R
  int64_t ncols_lids = 0;    // x length expected
  int64_t nnz = 0;           // owned-row nonzeros
  bool csr = false;          // built from a SparseMatrixCSR: α scales each product, (v*x)*α (SparseUtils.jl:247)
  // The main structure: the owned rows (nrows) in int32 columns; sl_all its
  // slices without / with ghost-column entries (d_bnd null: no boundary
  // slice, one launch over 0..nslices-1).  main.col16 / main.gbase: the
  // delta16 slices (below).  main.val continues past the slots (n_gnz, n_lnz).
  pa::Sell main;
  pa::SliceSet sl_all;
  // host copies for pa_mat_traffic and the build: int32-layout slice lengths,
  // pattern-layout slice kinds (BuildKind), entries per row of each
  // pattern-layout slice
  std::vector<int32_t> h_slen, h_kind, h_plen;
  // CSC nz p → its value: main slot (>= 0) or ghost-row value g (-(g+1)).
  // The ghost rows' nonzeros (stored by FE assembly, never multiplied) sit
  // after the SELL slots in main.val: the nz exchange/assemble (matrix
  // exchanger, Interfaces.jl:2312-2404) addresses both through one index.
  // Built by pa_mat_from_coo, the map stays on the device (d_nz_slot) until
  // a call that needs it on the host (set/get values, matrix exchanger).
  std::vector<int64_t> h_nz_slot;
  pa::DevBuf<int64_t> d_nz_slot;
  bool nz_map = false;              // built from a CSC pattern
  int64_t csc_nnz = 0;
  int64_t n_gnz = 0;
  // long rows (row-length histogram): their own CSR, values in main.val at
  // long_off = slots + n_gnz; CSC nz of a long row: h_nz_slot = -(n_gnz+t+1)
  int64_t n_long = 0, n_lnz = 0, long_off = 0;
  pa::DevBuf<int32_t> d_long_row;    // oids, ascending
  pa::DevBuf<int64_t> d_long_ptr;    // n_long+1
  pa::DevBuf<int32_t> d_long_col;    // x lids, reference order per row
  pa::DevBuf<int32_t> d_sflags;      // per slice: 1 if it holds long rows (int32 path skips them)
  pa::DevBuf<uint64_t> d_lmask;      // nslices*(H/64) bits: long rows
  std::vector<int32_t> h_long_rows;  // sorted oids (excluded from the side SELL)
  // chunks of the long rows (long_rows_exact = 0): chunk c covers long-CSR
  // entries [lchunk_start[c], lchunk_start[c+1]); row i owns chunks
  // [lrow_chunk[i], lrow_chunk[i+1]); one partial per chunk in d_lpart
  int64_t n_lchunks = 0;
  pa::DevBuf<int64_t> d_lchunk_start;
  pa::DevBuf<int64_t> d_lrow_chunk;
  pa::DevBuf<void> d_lpart;

  // Pattern slices (implied columns): in a pattern slice the
  // rows whose column sequence is `row + pat[k]` (k < plen) are "regular"
  // (mask bit set) and need no column ids; the other rows of the slice are
  // computed from the side SELL below.  Values keep their int32-SELL slots.
  bool has_pat = false;
  int kmax = 0;                      // pattern stride per slice
  pa::DevBuf<int32_t> d_kind;        // per slice: its BuildKind (the values the device copy holds: see the enum)
  pa::DevBuf<int32_t> d_pdesc;       // per slice desc_words(R) int32: {offset / H, d_plen, 0, 0, mask words} (SPMV_DESC)
  pa::DevBuf<int32_t> d_plen;        // per slice: entries per row (int32 len; pattern slices: len (bits 0-7) | tri flag (bit 8) | pattern id << 9)
  pa::DevBuf<int32_t> d_pat;         // npatterns*kmax offsets: the distinct patterns (dedup_patterns)
  int64_t npatterns = 0;
  // XCD run length of this matrix's per-kind launches in spmv_xcd_chunk's
  // auto mode (dedup_patterns: the pattern's reach in blocks / 8), 0 = none
  int xcd_auto = 0;
  pa::DevBuf<uint64_t> d_mask;       // nslices*(H/64) regular-row bits
  int64_t npattern_slices = 0, nregular_rows = 0;
  // the pattern layout's slices of the main structure by kind: pattern
  // slices, int32-column slices, and delta16 slices — int32-column slices
  // whose columns all fit a 16-bit code (pa_tune "spmv_delta16"): an owned
  // column c of row r as c - r in 15 signed bits, a ghost column as the
  // slice's ghost base + 15 unsigned bits (bit 15 set), 0xFFFF padding — 2 B
  // per slot instead of 4
  pa::SliceSet sl_pat, sl_i32, sl_d16;
  // longest row of each of those kinds (main.maxlen: of all slices)
  int maxlen_pat = INT32_MAX, maxlen_pm_int = INT32_MAX, maxlen_d16 = INT32_MAX;
  pa::Sell side;        // the irregular rows of pattern slices (row map → oid), int32 columns
  pa::TripleSell tri;
  pa::UniformRows uni;
  pa::DevBuf<void> d_dotp;  // fused dot: one partial per (main + side + triple) slice and long row

  // Entry views (pa_mat_scatter / pa_mat_gather).  The
  // builders that set nz_map keep the (row lid, col lid) of each ghost-row
  // nonzero (0-based, in the order of their values after the slots; a pair
  // of -1: an index out of range in a ghost row of a CSR parent), n_gnz * 8 B:
  // the only thing a matrix that never opens a view carries for them.  The
  // entry table is built by the first view call (mat_entry_table): the keys
  // row_lid * ncols_lids + col_lid of the stored entries, ascending, and each
  // entry's value index in main.val.
  int64_t nrows_lids = 0;
  pa::DevBuf<int32_t> d_ghost_rc;    // 2 * n_gnz
  bool has_entries = false;
  int64_t n_entries = 0;
  pa::DevBuf<uint64_t> d_ekey;       // n_entries
  pa::DevBuf<int64_t> d_eidx;        // n_entries
};

namespace pa {
// the call runs A's pattern layout: pattern, int32 and delta16 slices of the
// main structure, the side SELL and the triple SELL (else int32 slices only)
inline bool pattern_layout(const pa_mat* A) { return knobs().spmv_format == 1 && A->has_pat; }

// The fused dot's partials in pa_mat::d_dotp: one per slice of the main
// structure, then the side SELL's, the triple SELL's and one per long row.
// The kernels (SpmvArgs::dot_base) and the fold (SpmvCall::finish_part) both
// take the bases from here.
inline int64_t dot_base(const pa_mat* A, SliceKind k) {
  return k == kSide ? A->main.nslices : k == kTriple ? A->main.nslices + A->side.nslices : 0;
}
inline int64_t long_dot_base(const pa_mat* A) {
  return pattern_layout(A) ? dot_base(A, kTriple) + A->tri.nslices : A->main.nslices;
}

// The entry views of a matrix (pa_coo.hip; pa_mat_scatter / pa_mat_gather).
// mat_entry_table builds A's entry table from its layout (rows: the index
// set of the matrix's rows); 0, or -1 on a HIP error.  mat_entry_ids writes
// the 1-based value index in main.val of each (I[k], J[k]) to vidx (0: no
// such value) — I, J, vidx device arrays, ids as in pa::vec_scatter, looked
// up in rows / cols — and returns 1 when an id has no lid (absent_zero: an
// absent global id is no error), 2 when `stored` and a valid (i, j) is not
// stored, -1 on a HIP error.  Both have completed on st when they return.
int mat_entry_table(pa_mat* A, const pa_index* rows, hipStream_t st);
int mat_entry_ids(const pa_mat* A, const pa_index* rows, const pa_index* cols, bool global, int index_bytes,
                  bool absent_zero, bool stored, int64_t n, const void* I, const void* J, int64_t* vidx,
                  hipStream_t st);
// pa_mat_findnz (pa_coo.hip): the stored entries of A — of its owned rows, or
// of every stored row — into out in the parent's storage order, ids as
// 1-based lids or (global) gids through the lid_to_gid of rows / cols; 0, or
// -1 on a HIP error.  The work has completed on st when it returns.
int mat_findnz(const pa_mat* A, const pa_index* rows, const pa_index* cols, bool owned_only, bool global,
               CooList& out, hipStream_t st);
}  // namespace pa

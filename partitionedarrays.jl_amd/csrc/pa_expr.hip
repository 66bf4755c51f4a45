// pa_expr.hip — broadcast expressions over PVector parts (pa_vec_eval,
// pa_reduce_expr_all; Interfaces.jl:1688-1765, 1682-1686, 1767-1863).
//
// One evaluator (expr_run) interprets the postfix program of include/pa_hip.h
// per element; two kernels per element type use it: evaluate-and-store and
// evaluate-and-reduce.  The program is a by-value kernel argument, hence
// wave-uniform: every branch of the interpreter is a scalar branch.
//
// No scratch: the operand stack is a fixed file of PA_EXPR_MAX_DEPTH slots
// whose top is always slot 0 — a push shifts the slots up, a binary op
// shifts them down — so every slot index is a compile-time constant and the
// stack lives in VGPRs (DESIGN.md §4.4 has the resource-usage lines).  The
// operands of a step are loaded up front into their own registers (a fixed
// file as well, read by a uniform switch), so one step has every operand's
// load in flight at once.
//
// Types: a slot holds the wide type W = wide_of<T> (double / c128).  An op
// tagged T narrows its operands (exactly: they are T values), computes in T
// and widens the result; an op tagged PA_EXPR_WIDE computes in W.  The store
// rounds to T once.  Compiled with -ffp-contract=off like the whole library;
// Float32 division is hipcc's correctly rounded sequence.
#include "pa_internal.h"

#include <type_traits>

namespace pa {
namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kDepth = PA_EXPR_MAX_DEPTH;
constexpr int kVecs = PA_EXPR_MAX_VECS;

template <typename T> struct is_cplx : std::false_type {};
template <> struct is_cplx<c64> : std::true_type {};
template <> struct is_cplx<c128> : std::true_type {};
// the component type an op of T computes in (C = float / double)
template <typename T> struct comp_of { using type = typename real_of<T>::type; };

template <typename T, int E> struct alignas(16) Pack { T v[E]; };

// ---- one op on one element: real nodes (double slots) ---------------------
template <typename C> __device__ inline double r_arith(int code, double a, double b) {
  const C x = (C)a, y = (C)b;
  switch (code) {
    case PA_OP_ADD: return (double)(x + y);
    case PA_OP_SUB: return (double)(x - y);
    case PA_OP_MUL: return (double)(x * y);
    default: return (double)(x / y);  // PA_OP_DIV
  }
}
// comparisons: the operands are exact in either type, so Float64 compares
__device__ inline double r_cmp(int code, double a, double b) {
  bool t;
  switch (code) {
    case PA_OP_LT: t = a < b; break;
    case PA_OP_LE: t = a <= b; break;
    case PA_OP_GT: t = a > b; break;
    case PA_OP_GE: t = a >= b; break;
    case PA_OP_EQ: t = a == b; break;
    default: t = a != b; break;  // PA_OP_NE
  }
  return t ? 1.0 : 0.0;
}

// ---- complex nodes (c128 slots); lr / rr: the left / right operand is real
// valued (im = 0), Julia's Real ∘ Complex methods (base/complex.jl) ----------
template <typename C> __device__ inline c128 c_arith(int code, c128 a, c128 b, bool lr, bool rr) {
  const C ar = (C)a.re, ai = (C)a.im, br = (C)b.re, bi = (C)b.im;
  switch (code) {
    case PA_OP_ADD:
      return c128{(double)(ar + br), lr ? (rr ? 0.0 : (double)bi) : rr ? (double)ai : (double)(ai + bi)};
    case PA_OP_SUB:
      return c128{(double)(ar - br), lr ? (rr ? 0.0 : (double)(-bi)) : rr ? (double)ai : (double)(ai - bi)};
    case PA_OP_MUL:
      if (lr) return c128{(double)(ar * br), rr ? 0.0 : (double)(ar * bi)};
      if (rr) return c128{(double)(ar * br), (double)(ai * br)};
      return c128{(double)(ar * br - ai * bi), (double)(ar * bi + ai * br)};
    default:  // PA_OP_DIV: real operands only (pa_expr_check)
      return c128{(double)(ar / br), 0.0};
  }
}
__device__ inline c128 c_cmp(int code, c128 a, c128 b) {
  if (code == PA_OP_EQ) return c128{(a.re == b.re && a.im == b.im) ? 1.0 : 0.0, 0.0};
  if (code == PA_OP_NE) return c128{(a.re == b.re && a.im == b.im) ? 0.0 : 1.0, 0.0};
  return c128{r_cmp(code, a.re, b.re), 0.0};  // ordered: real operands only
}

template <typename T, typename C, typename W>
__device__ inline W binary(int code, int fl, W a, W b) {
  if constexpr (is_cplx<T>::value) {
    if (code >= PA_OP_LT) return c_cmp(code, a, b);
    return c_arith<C>(code, a, b, (fl & PA_EXPR_LREAL) != 0, (fl & PA_EXPR_RREAL) != 0);
  } else {
    if (code >= PA_OP_LT) return r_cmp(code, a, b);
    return r_arith<C>(code, a, b);
  }
}

template <typename T, typename C, typename W>
__device__ inline W unary(int code, int fl, W a) {
  if constexpr (is_cplx<T>::value) {
    const bool real = (fl & PA_EXPR_LREAL) != 0;
    const C ar = (C)a.re, ai = (C)a.im;
    switch (code) {
      case PA_OP_NEG: return c128{-a.re, real ? 0.0 : -a.im};
      case PA_OP_ABS: return c128{__builtin_fabs(a.re), 0.0};  // real operands only
      case PA_OP_ABS2: return c128{real ? (double)(ar * ar) : (double)(ar * ar + ai * ai), 0.0};
      default: return c128{a.re, real ? 0.0 : -a.im};  // PA_OP_CONJ
    }
  } else {
    const C x = (C)a;
    switch (code) {
      case PA_OP_NEG: return -a;
      case PA_OP_ABS: return __builtin_fabs(a);
      case PA_OP_ABS2: return (double)(x * x);
      default: return a;  // PA_OP_CONJ
    }
  }
}

template <typename W> __device__ inline W scal_as(const c128& s) {
  if constexpr (std::is_same<W, c128>::value) return s; else return s.re;
}

// ---- operand loads --------------------------------------------------------
// fast path: step i of operand k is the 16 bytes at v[k] + 16 i (non-temporal,
// as the SpMV's streams)
template <typename T, int E>
__device__ inline void load_fast(const ExprArgs& a, int64_t i, T (&in)[kVecs][E]) {
#pragma unroll
  for (int k = 0; k < kVecs; ++k) {
    if (k < a.nvec) {
      const Pack<T, E> p = __builtin_bit_cast(Pack<T, E>, __builtin_nontemporal_load((const u32x4*)a.v[k] + i));
#pragma unroll
      for (int e = 0; e < E; ++e) in[k][e] = p.v[e];
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) in[k][e] = zero_of<T>();
    }
  }
}
// one element per lane, through each operand's own map
template <typename T>
__device__ inline void load_elem(const ExprArgs& a, int64_t i, T (&in)[kVecs][1]) {
#pragma unroll
  for (int k = 0; k < kVecs; ++k) {
    if (k < a.nvec) {
      const int32_t* m = a.map[k];
      in[k][0] = ((const T*)a.v[k])[m ? (int64_t)m[i] : i];
    } else {
      in[k][0] = zero_of<T>();
    }
  }
}

// ---- the evaluator: E elements per lane ----------------------------------
template <typename T, int E>
__device__ inline void expr_run(const ExprArgs& a, const T (&in)[kVecs][E], typename wide_of<T>::type (&out)[E]) {
  using W = typename wide_of<T>::type;
  using C = typename comp_of<T>::type;    // narrow component type
  using CW = typename comp_of<W>::type;   // double
  W s[kDepth][E];
#pragma unroll
  for (int d = 0; d < kDepth; ++d)
#pragma unroll
    for (int e = 0; e < E; ++e) s[d][e] = zero_of<W>();
  const int nops = a.prog.nops;
  for (int pc = 0; pc < nops; ++pc) {
    const pa_expr_op op = a.prog.ops[pc];
    const int code = op.code, fl = op.flags, mode = op.flags & PA_EXPR_MODE;
    if (code <= PA_OP_SCAL) {  // push
      W x[E];
      if (code == PA_OP_SCAL) {
        const W c = scal_as<W>(a.scal[op.arg]);
#pragma unroll
        for (int e = 0; e < E; ++e) x[e] = c;
      } else {
        switch (op.arg) {
#define PA_EXPR_PUSH(K)                                   \
  case K:                                                 \
    _Pragma("unroll") for (int e = 0; e < E; ++e) x[e] = widen(in[K][e]); \
    break;
          PA_EXPR_PUSH(0) PA_EXPR_PUSH(1) PA_EXPR_PUSH(2) PA_EXPR_PUSH(3)
          PA_EXPR_PUSH(4) PA_EXPR_PUSH(5) PA_EXPR_PUSH(6)
          default:
            _Pragma("unroll") for (int e = 0; e < E; ++e) x[e] = widen(in[7][e]);
            break;
#undef PA_EXPR_PUSH
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
#pragma unroll
        for (int d = kDepth - 1; d >= 1; --d) s[d][e] = s[d - 1][e];
        s[0][e] = x[e];
      }
    } else if (code >= PA_OP_NEG && code <= PA_OP_CONJ) {
      if (std::is_same<T, W>::value || (fl & PA_EXPR_WIDE)) {
#pragma unroll
        for (int e = 0; e < E; ++e) s[0][e] = unary<T, CW, W>(code, fl, s[0][e]);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) s[0][e] = unary<T, C, W>(code, fl, s[0][e]);
      }
    } else {  // binary: left ∘ right by operand mode
      W l[E], r[E];
      if (mode == PA_EXPR_SS || mode == PA_EXPR_RS) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          l[e] = mode == PA_EXPR_SS ? s[1][e] : s[0][e];
          r[e] = mode == PA_EXPR_SS ? s[0][e] : s[1][e];
#pragma unroll
          for (int d = 1; d < kDepth - 1; ++d) s[d][e] = s[d + 1][e];
        }
      } else {
        const W c = scal_as<W>(a.scal[op.arg]);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          l[e] = mode == PA_EXPR_SC ? s[0][e] : c;
          r[e] = mode == PA_EXPR_SC ? c : s[0][e];
        }
      }
      if (std::is_same<T, W>::value || (fl & PA_EXPR_WIDE)) {
#pragma unroll
        for (int e = 0; e < E; ++e) s[0][e] = binary<T, CW, W>(code, fl, l[e], r[e]);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) s[0][e] = binary<T, C, W>(code, fl, l[e], r[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) out[e] = s[0][e];
}

// ---- evaluate and store ---------------------------------------------------
// Fast path (every operand and y identity-addressed from a 16 B aligned
// base): grid-stride over the n / E whole 16 B steps, then the up to E - 1
// tail elements one per lane.
template <typename T>
__global__ __launch_bounds__(256) void k_expr_store(int64_t n, ExprArgs a, T* y) {
  using W = typename wide_of<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nsteps = n / E;
  for (int64_t i = tid; i < nsteps; i += (int64_t)gridDim.x * blockDim.x) {
    T in[kVecs][E];
    load_fast<T, E>(a, i, in);
    W r[E];
    expr_run<T, E>(a, in, r);
    Pack<T, E> o;
#pragma unroll
    for (int e = 0; e < E; ++e) o.v[e] = narrow<T>(r[e]);
    *((u32x4*)y + i) = __builtin_bit_cast(u32x4, o);
  }
  if constexpr (E > 1) {
    const int64_t t = nsteps * E + tid;
    if (t < n) {
      T in[kVecs][1];
      load_elem<T>(a, t, in);  // maps are null on this path
      W r[1];
      expr_run<T, 1>(a, in, r);
      y[t] = narrow<T>(r[0]);
    }
  }
}

// Mapped path: one element per lane, gathered through each operand's map.
template <typename T>
__global__ __launch_bounds__(256) void k_expr_store_map(int64_t n, ExprArgs a, T* y,
                                                        const int32_t* __restrict__ ymap) {
  using W = typename wide_of<T>::type;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    T in[kVecs][1];
    load_elem<T>(a, i, in);
    W r[1];
    expr_run<T, 1>(a, in, r);
    y[ymap ? (int64_t)ymap[i] : i] = narrow<T>(r[0]);
  }
}

// ---- evaluate and reduce --------------------------------------------------
// SUM accumulates in W (double / c128, pa_sum_all's accumulators); MAX / MIN
// in double over the real part (real-valued expressions only), a NaN wins,
// and of two equal values Julia's max / min pick +0.0 / -0.0.
template <typename T, int KIND> struct red_of { using type = double; };
template <typename T> struct red_of<T, PA_REDUCE_SUM> { using type = typename wide_of<T>::type; };

template <int KIND, typename A> __device__ inline A red_init() {
  if constexpr (KIND == PA_REDUCE_SUM) return zero_of<A>();
  else return KIND == PA_REDUCE_MAX ? -__builtin_huge_val() : __builtin_huge_val();
}
template <int KIND, typename A> __device__ inline A red_comb(A a, A b) {
  if constexpr (KIND == PA_REDUCE_SUM) {
    return a + b;
  } else {
    if (a != a) return a;
    if (b != b) return b;
    if (KIND == PA_REDUCE_MAX) return a > b ? a : b > a ? b : (__builtin_signbit(a) ? b : a);
    return a < b ? a : b < a ? b : (__builtin_signbit(a) ? a : b);
  }
}
template <int KIND, typename A, typename W> __device__ inline A red_val(W v) {
  if constexpr (KIND == PA_REDUCE_SUM) return v;
  else if constexpr (std::is_same<W, c128>::value) return v.re;
  else return v;
}

// block_reduce's tree (pa_internal.h) with the kind's combine: wave tree, then
// waves 0..3 in order; valid on thread 0
template <int KIND, typename A>
__device__ inline A block_fold(A v) {
  __shared__ A sm[4];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = red_comb<KIND>(v, shfl_down64(v, d));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  A r = red_init<KIND, A>();
  if (threadIdx.x == 0) {
    r = sm[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = red_comb<KIND>(r, sm[i]);
  }
  return r;
}

template <typename T, int KIND, bool FAST>
__global__ __launch_bounds__(256) void k_expr_reduce(int64_t n, ExprArgs a, typename red_of<T, KIND>::type* out,
                                                     typename red_of<T, KIND>::type* __restrict__ result,
                                                     unsigned* ticket) {
  using W = typename wide_of<T>::type;
  using A = typename red_of<T, KIND>::type;
  constexpr int E = FAST ? 16 / (int)sizeof(T) : 1;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  A acc = red_init<KIND, A>();
  const int64_t nsteps = n / E;
  for (int64_t i = tid; i < nsteps; i += (int64_t)gridDim.x * blockDim.x) {
    T in[kVecs][E];
    if constexpr (FAST) load_fast<T, E>(a, i, in); else load_elem<T>(a, i, in);
    W r[E];
    expr_run<T, E>(a, in, r);
#pragma unroll
    for (int e = 0; e < E; ++e) acc = red_comb<KIND>(acc, red_val<KIND, A>(r[e]));
  }
  if constexpr (E > 1) {
    const int64_t t = nsteps * E + tid;
    if (t < n) {
      T in[kVecs][1];
      load_elem<T>(a, t, in);
      W r[1];
      expr_run<T, 1>(a, in, r);
      acc = red_comb<KIND>(acc, red_val<KIND, A>(r[0]));
    }
  }
  // block partials to out[blockIdx]; the last block folds them in block order
  // (k_reduce_partial's hand-off)
  A r = block_fold<KIND>(acc);
  if (!publish_arrive(out, r, ticket)) return;
  A f = red_init<KIND, A>();
  for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) f = red_comb<KIND>(f, ld_wt(&out[i]));
  f = block_fold<KIND>(f);
  if (threadIdx.x == 0) result[0] = f;
}

constexpr int kStoreBlocks = 8192;   // launch_axpby's cap
constexpr int kReduceBlocks = 1024;  // launch_reduce's cap (the partials buffer holds 8192)

int grid_for(int64_t n, int64_t cap) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

template <typename T>
void store_t(int64_t n, const ExprArgs& a, void* y, const int32_t* ymap, bool fast, hipStream_t st) {
  if (fast) {
    constexpr int E = 16 / (int)sizeof(T);
    hipLaunchKernelGGL(k_expr_store<T>, dim3(grid_for(n / E, kStoreBlocks)), dim3(256), 0, st, n, a, (T*)y);
  } else {
    hipLaunchKernelGGL(k_expr_store_map<T>, dim3(grid_for(n, kStoreBlocks)), dim3(256), 0, st, n, a, (T*)y, ymap);
  }
}

template <typename T, int KIND>
void reduce_tk(int64_t n, const ExprArgs& a, bool fast, void* partials, void* result, unsigned* ticket,
               hipStream_t st) {
  using A = typename red_of<T, KIND>::type;
  if (fast) {
    constexpr int E = 16 / (int)sizeof(T);
    hipLaunchKernelGGL((k_expr_reduce<T, KIND, true>), dim3(grid_for(n / E, kReduceBlocks)), dim3(256), 0, st, n, a,
                       (A*)partials, (A*)result, ticket);
  } else {
    hipLaunchKernelGGL((k_expr_reduce<T, KIND, false>), dim3(grid_for(n, kReduceBlocks)), dim3(256), 0, st, n, a,
                       (A*)partials, (A*)result, ticket);
  }
}
template <typename T>
void reduce_t(int kind, int64_t n, const ExprArgs& a, bool fast, void* partials, void* result, unsigned* ticket,
              hipStream_t st) {
  if (kind == PA_REDUCE_SUM) reduce_tk<T, PA_REDUCE_SUM>(n, a, fast, partials, result, ticket, st);
  else if (kind == PA_REDUCE_MAX) reduce_tk<T, PA_REDUCE_MAX>(n, a, fast, partials, result, ticket, st);
  else reduce_tk<T, PA_REDUCE_MIN>(n, a, fast, partials, result, ticket, st);
}

}  // namespace

void launch_expr_store(int dtype, int64_t n, const ExprArgs& a, void* y, const int32_t* ymap, bool fast,
                       hipStream_t st) {
  if (n <= 0) return;
  switch (dtype) {
    case PA_F32: store_t<float>(n, a, y, ymap, fast, st); break;
    case PA_F64: store_t<double>(n, a, y, ymap, fast, st); break;
    case PA_C64: store_t<c64>(n, a, y, ymap, fast, st); break;
    case PA_C128: store_t<c128>(n, a, y, ymap, fast, st); break;
  }
}

// n == 0 still launches: the part's value is the kind's init
void launch_expr_reduce(int dtype, int kind, int64_t n, const ExprArgs& a, bool fast, void* partials,
                        void* result, unsigned* ticket, hipStream_t st) {
  switch (dtype) {
    case PA_F32: reduce_t<float>(kind, n, a, fast, partials, result, ticket, st); break;
    case PA_F64: reduce_t<double>(kind, n, a, fast, partials, result, ticket, st); break;
    case PA_C64: reduce_t<c64>(kind, n, a, fast, partials, result, ticket, st); break;
    case PA_C128: reduce_t<c128>(kind, n, a, fast, partials, result, ticket, st); break;
  }
}

}  // namespace pa

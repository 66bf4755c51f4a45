// pa_pcg.hip — Jacobi-preconditioned CG (pa_mat_diag, pa_pcg_apply_all,
// pa_pcg_update_all, pa_pcg_solve_all): diag(A) read off the
// SELL layout, the preconditioner's apply fused with ρ = dot(c, r), the tail
// of one iteration fused with the head of the next, and the kernels of the
// device-driven recurrence (its scalars in a PCGState).
//
// Float32 and Float64 only.  Every element is evaluated in T, rounded at
// every operation (the library is compiled with -ffp-contract=off; `/` is
// hipcc's correctly rounded division): what Julia's ldiv!(c, Diagonal(d), r)
// and the broadcasts x .+= α.*u, r .-= α.*c with α::T compute per element.
#include "pa_internal.h"

#include <algorithm>

namespace pa {
namespace {

template <typename T, int E> struct alignas(sizeof(T) * E) Pack { T v[E]; };

// ---- diag(A) ---------------------------------------------------------------
// what k_mat_diag reads of a matrix (the walk of k_entry_emit, pa_coo.hip,
// by row instead of by value index)
struct DiagSrc {
  int64_t nrows, nslices, slots, n_long, long_off, nd;
  int H, R;
  const int64_t* off;         // main.off
  const int32_t* col;         // main.col
  const int32_t* kind;        // pa_mat::d_kind (null: every slice blocked)
  const int32_t* own;         // the columns' oid_to_lid, 0-based (null: the identity)
  const int32_t* long_row;
  const int64_t* long_ptr;
  const int32_t* long_col;
};

// Owned row oid sits in slice s = oid / H at position w = oid % H: lane
// w / R, row-in-lane w % R — or lane w % 64, row-in-lane w / 64 in a Float32
// delta16 slice of 4 rows per lane (k_delta16 moved its rows) — and its entry
// k at value index off[s] + (k*64 + lane)*R + rr.  The slices are contiguous,
// so the entries per row of slice s are (off[s+1] - off[s]) / H.  The row's
// own column is the lid of owned id oid in the columns' index set.  One
// thread per row; each row has at most one such entry, so every write is
// unique.  Padding slots hold column -1 and a long row's slots are padding.
template <typename T>
__global__ __launch_bounds__(256) void k_mat_diag(DiagSrc a, const T* __restrict__ val, T* __restrict__ d) {
  for (int64_t oid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; oid < a.nrows;
       oid += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = oid / a.H;
    const int w = (int)(oid % a.H);
    const bool il = a.R == 4 && a.kind && a.kind[s] == kBkDelta16;
    const int lane = il ? w % 64 : w / a.R, rr = il ? w / 64 : w % a.R;
    const int64_t lo = a.off[s], hi = s + 1 < a.nslices ? a.off[s + 1] : a.slots;
    const int64_t len = (hi - lo) / a.H;
    const int64_t target = a.own ? (int64_t)a.own[oid] : oid;
    if (target < 0 || target >= a.nd) continue;
    for (int64_t k = 0; k < len; ++k) {
      const int64_t t = lo + (k * 64 + lane) * a.R + rr;
      if (a.col[t] == target) {
        d[target] = val[t];
        break;
      }
    }
  }
}

// the long rows (their own CSR, values at long_off): one wave per row, the
// lanes striding over the row's entries
template <typename T>
__global__ __launch_bounds__(256) void k_mat_diag_long(DiagSrc a, const T* __restrict__ val, T* __restrict__ d) {
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= a.n_long) return;
  const int64_t oid = a.long_row[wave];
  const int64_t target = a.own ? (int64_t)a.own[oid] : oid;
  if (target < 0 || target >= a.nd) return;
  for (int64_t q = a.long_ptr[wave] + lane; q < a.long_ptr[wave + 1]; q += 64)
    if (a.long_col[q] == target) d[target] = val[a.long_off + q];
}

template <typename T>
void mat_diag_t(const DiagSrc& a, const void* val, void* d, hipStream_t st) {
  if (a.nrows > 0 && a.slots > 0) {
    const int nb = (int)std::min<int64_t>(8192, (a.nrows + 255) / 256);
    hipLaunchKernelGGL(k_mat_diag<T>, dim3(nb), dim3(256), 0, st, a, (const T*)val, (T*)d);
  }
  if (a.n_long > 0) {
    const int nb = (int)((a.n_long + 3) / 4);
    hipLaunchKernelGGL(k_mat_diag_long<T>, dim3(nb), dim3(256), 0, st, a, (const T*)val, (T*)d);
  }
}

// ---- c = r ./ d and ρ = dot(c, r) -----------------------------------------
// All lids; the owned Σ c_i*r_i (contiguous owned lids 0..noids-1; product in
// T, accumulated in Float64 as k_reduce_partial does) as per-block partials,
// folded in block order afterwards.  V elements per 16 B access (V = 1:
// unaligned fallback).  c may be r or d: each lane reads its index before it
// writes it.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_pcg_apply(int64_t n, int64_t noids, T* c, const T* r, const T* d,
                                                   double* __restrict__ part) {
  using P = Pack<T, V>;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nv = n / V;
  double s = 0.0;
  for (int64_t j = t; j < nv; j += stride) {
    const P rv = reinterpret_cast<const P*>(r)[j];
    const P dv = reinterpret_cast<const P*>(d)[j];
    P cv;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      cv.v[e] = rv.v[e] / dv.v[e];
      if (j * V + e < noids) s = s + (double)(cv.v[e] * rv.v[e]);
    }
    reinterpret_cast<P*>(c)[j] = cv;
  }
  for (int64_t i = nv * V + t; i < n; i += stride) {
    const T ri = r[i];
    const T ci = ri / d[i];
    c[i] = ci;
    if (i < noids) s = s + (double)(ci * ri);
  }
  const double b = block_reduce(s);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

template <typename T>
void pcg_apply_t(int64_t n, int64_t noids, void* c, const void* r, const void* d, double* part, int nb,
                 hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const bool aligned = ((uintptr_t)c | (uintptr_t)r | (uintptr_t)d) % 16 == 0;
  if (aligned)
    hipLaunchKernelGGL((k_pcg_apply<T, V>), dim3(nb), dim3(256), 0, st, n, noids, (T*)c, (const T*)r, (const T*)d,
                       part);
  else
    hipLaunchKernelGGL((k_pcg_apply<T, 1>), dim3(nb), dim3(256), 0, st, n, noids, (T*)c, (const T*)r, (const T*)d,
                       part);
}

// ---- x .+= α.*u; r .-= α.*c; c = r ./ d; norm(r)², dot(c, r) -------------
// One pass over all lids, α of the element type; c is A*u on entry and the
// preconditioned new residual on exit, read and written at the same index by
// the same lane.  The owned Σ r_i² (.re) and Σ c_i*r_i (.im) of the new
// values as one c128 partial per block (contiguous owned lids 0..noids-1).
// DEV: α comes from the device PCG state (pa_pcg_solve_all) and a finished
// solve is a no-op.
template <typename T, int V, bool DEV>
__global__ __launch_bounds__(256) void k_pcg_update(int64_t n, int64_t noids, T* __restrict__ x, T* __restrict__ r,
                                                    const T* __restrict__ u, T* __restrict__ c,
                                                    const T* __restrict__ d, T alpha,
                                                    const PCGState* __restrict__ st, c128* __restrict__ part) {
  if (DEV) {
    if (st->done) return;
    alpha = (T)st->alpha;
  }
  using P = Pack<T, V>;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nv = n / V;
  c128 s{0.0, 0.0};
  for (int64_t j = t; j < nv; j += stride) {
    P xv = reinterpret_cast<const P*>(x)[j];
    const P uv = reinterpret_cast<const P*>(u)[j];
    P rv = reinterpret_cast<const P*>(r)[j];
    P cv = reinterpret_cast<const P*>(c)[j];
    const P dv = reinterpret_cast<const P*>(d)[j];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      xv.v[e] = xv.v[e] + alpha * uv.v[e];
      rv.v[e] = rv.v[e] - alpha * cv.v[e];
      cv.v[e] = rv.v[e] / dv.v[e];
      if (j * V + e < noids) s = s + c128{(double)(rv.v[e] * rv.v[e]), (double)(cv.v[e] * rv.v[e])};
    }
    reinterpret_cast<P*>(x)[j] = xv;
    reinterpret_cast<P*>(r)[j] = rv;
    reinterpret_cast<P*>(c)[j] = cv;
  }
  for (int64_t i = nv * V + t; i < n; i += stride) {
    x[i] = x[i] + alpha * u[i];
    const T ri = r[i] - alpha * c[i];
    const T ci = ri / d[i];
    r[i] = ri;
    c[i] = ci;
    if (i < noids) s = s + c128{(double)(ri * ri), (double)(ci * ri)};
  }
  const c128 b = block_reduce(s);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

template <typename T>
void pcg_update_t(int64_t n, int64_t noids, void* x, void* r, const void* u, void* c, const void* d,
                  const void* alpha, const PCGState* cst, c128* part, int nb, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const bool aligned = ((uintptr_t)x | (uintptr_t)r | (uintptr_t)u | (uintptr_t)c | (uintptr_t)d) % 16 == 0;
  const T a = alpha ? *(const T*)alpha : T(0);
#define PA_PU(VV, DD)                                                                                           \
  hipLaunchKernelGGL((k_pcg_update<T, VV, DD>), dim3(nb), dim3(256), 0, st, n, noids, (T*)x, (T*)r, (const T*)u, \
                     (T*)c, (const T*)d, a, cst, part)
  if (cst) {
    if (aligned) PA_PU(V, true); else PA_PU(1, true);
  } else {
    if (aligned) PA_PU(V, false); else PA_PU(1, false);
  }
#undef PA_PU
}

// ---- the device-driven recurrence (pa_pcg_solve_all) -----------------------
// The same arithmetic as the host-driven fused loop (pvector._pcg over
// pa_vec_axpby, pa_spmv_dot_all and pa_pcg_update_all), the scalars on one
// thread, so the device recurrence equals it bit for bit.

// u .= c .+ β.*u over all lids, β = ρ/ρ_prev: one division in T, then per
// element the product and the sum each rounded in T (pa_vec_axpby mode 0 with
// a scalar of the element type).  A finished solve is a no-op.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_pcg_xu(int64_t n, T* __restrict__ u, const T* __restrict__ c,
                                                const PCGState* __restrict__ st) {
  if (st->done) return;
  const T b = (T)st->rho / (T)st->rho_prev;
  using P = Pack<T, V>;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nv = n / V;
  for (int64_t j = t; j < nv; j += stride) {
    P uv = reinterpret_cast<const P*>(u)[j];
    const P cv = reinterpret_cast<const P*>(c)[j];
#pragma unroll
    for (int e = 0; e < V; ++e) uv.v[e] = cv.v[e] + b * uv.v[e];
    reinterpret_cast<P*>(u)[j] = uv;
  }
  for (int64_t i = nv * V + t; i < n; i += stride) u[i] = c[i] + b * u[i];
}

template <typename T>
void pcg_xu_t(int64_t n, void* u, const void* c, const PCGState* cst, hipStream_t st) {
  constexpr int V = 16 / sizeof(T);
  const bool aligned = ((uintptr_t)u | (uintptr_t)c) % 16 == 0;
  const int64_t nw = aligned ? (n + V - 1) / V : n;
  const int nb = (int)std::min<int64_t>(8192, std::max<int64_t>(1, (nw + 255) / 256));
  if (aligned) hipLaunchKernelGGL((k_pcg_xu<T, V>), dim3(nb), dim3(256), 0, st, n, (T*)u, (const T*)c, cst);
  else hipLaunchKernelGGL((k_pcg_xu<T, 1>), dim3(nb), dim3(256), 0, st, n, (T*)u, (const T*)c, cst);
}

// the dot(u, c) values of the P parts (Float64 accumulators, part order) →
// dot = reduce(+; init=zero(T)) over the part values, each rounded to T
// (fold_parts, pa_api.cpp) → α = ρ / dot, one division in T
template <typename T>
__global__ void k_pcg_alpha(int P, const double* __restrict__ gathered, PCGState* __restrict__ st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (st->done) return;
  T s = (T)0;
  for (int p = 0; p < P; ++p) s = s + (T)gathered[p];
  st->alpha = (double)((T)st->rho / s);
}

// the {Σr², Σc·r} values of the P parts → both folded as above;
// residual = sqrt(Σr²) in Float64; ρ_prev = ρ; ρ = Σc·r; it += 1;
// history[it-1] = residual; done = it >= maxiter || residual <= tol (a NaN
// residual never satisfies <=: such a solve runs to maxiter, as on the host).
template <typename T>
__global__ void k_pcg_step(int P, const c128* __restrict__ gathered, PCGState* __restrict__ st,
                           double* __restrict__ history) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (st->done) return;
  T rr = (T)0, cr = (T)0;
  for (int p = 0; p < P; ++p) {
    rr = rr + (T)gathered[p].re;
    cr = cr + (T)gathered[p].im;
  }
  const double res = sqrt((double)rr);
  st->res = res;
  st->rho_prev = st->rho;
  st->rho = (double)cr;
  const int64_t it = st->it + 1;
  st->it = it;
  if (history) history[it - 1] = res;
  st->done = (it >= st->maxiter || res <= st->tol) ? 1 : 0;
}

}  // namespace

// d (nd values, zeroed by the caller on st) takes the stored diagonal of A's
// owned rows; own: the 0-based oid_to_lid of the columns' index set (null:
// the identity).  Real element types only.
void launch_mat_diag(const pa_mat* A, const int32_t* own, void* d, int64_t nd, hipStream_t st) {
  DiagSrc a;
  a.nrows = A->main.nrows, a.nslices = A->main.nslices, a.slots = A->main.slots;
  a.n_long = A->n_long, a.long_off = A->long_off, a.nd = nd;
  a.H = A->H, a.R = A->R;
  a.off = A->main.off, a.col = A->main.col, a.kind = A->d_kind, a.own = own;
  a.long_row = A->d_long_row, a.long_ptr = A->d_long_ptr, a.long_col = A->d_long_col;
  if (A->dtype == PA_F32) mat_diag_t<float>(a, A->main.val, d, st);
  else mat_diag_t<double>(a, A->main.val, d, st);
}

// c = r ./ d over n lids; part[0..nb-1]: the blocks' Σ c_i*r_i over lids < noids
void launch_pcg_apply(int dtype, int64_t n, int64_t noids, void* c, const void* r, const void* d, double* part,
                      int nb, hipStream_t st) {
  if (dtype == PA_F32) pcg_apply_t<float>(n, noids, c, r, d, part, nb, st);
  else pcg_apply_t<double>(n, noids, c, r, d, part, nb, st);
}

// alpha: host scalar of the element type (cst null), or read from the device
// PCG state; part[0..nb-1]: the blocks' {Σ r_i², Σ c_i*r_i} over lids < noids
void launch_pcg_update(int dtype, int64_t n, int64_t noids, void* x, void* r, const void* u, void* c, const void* d,
                       const void* alpha, const PCGState* cst, void* part, int nb, hipStream_t st) {
  if (dtype == PA_F32) pcg_update_t<float>(n, noids, x, r, u, c, d, alpha, cst, (c128*)part, nb, st);
  else pcg_update_t<double>(n, noids, x, r, u, c, d, alpha, cst, (c128*)part, nb, st);
}

void launch_pcg_xu(int dtype, int64_t n, void* u, const void* c, const PCGState* cst, hipStream_t st) {
  if (dtype == PA_F32) pcg_xu_t<float>(n, u, c, cst, st);
  else pcg_xu_t<double>(n, u, c, cst, st);
}

// gathered: P Float64 values (the parts' dot(u, c))
void launch_pcg_alpha(int dtype, int P, const void* gathered, PCGState* cst, hipStream_t st) {
  if (dtype == PA_F32) hipLaunchKernelGGL(k_pcg_alpha<float>, dim3(1), dim3(64), 0, st, P, (const double*)gathered, cst);
  else hipLaunchKernelGGL(k_pcg_alpha<double>, dim3(1), dim3(64), 0, st, P, (const double*)gathered, cst);
}

// gathered: P c128 values (the parts' {Σr², Σc·r})
void launch_pcg_step(int dtype, int P, const void* gathered, PCGState* cst, double* history, hipStream_t st) {
  if (dtype == PA_F32)
    hipLaunchKernelGGL(k_pcg_step<float>, dim3(1), dim3(64), 0, st, P, (const c128*)gathered, cst, history);
  else
    hipLaunchKernelGGL(k_pcg_step<double>, dim3(1), dim3(64), 0, st, P, (const c128*)gathered, cst, history);
}

}  // namespace pa

// pa_table.hip — the derived exchanger of a Table on the device.
//
// Reference: async_exchange!(combine_op, values::AbstractPData{<:Table},
// exchanger) (Interfaces.jl:899-908) → _table_exchanger / _table_lids_snd
// (920-961): every lid of lids_rcv / lids_snd is replaced by the data
// positions of its row, tptrs[lid] .. tptrs[lid+1]-1, and the vector exchange
// runs over the table's data with those lists.
//
// Here one side of the base exchanger (slots s = 0..n-1, lids l[s], neighbour
// offsets P[j]) and the table offsets t (0-based, nrows+1) give
//   len[s] = t[l[s]+1] - t[l[s]],  E = exclusive_scan(len)  (E[n] the total),
//   expanded lid E[s] + i = t[l[s]] + i  for i < len[s],
//   expanded neighbour offsets P'[j] = E[P[j]]  (all the host reads back),
// and the ordered combine plan of the side (target T[k], its slots
// pos[ptr[k] .. ptr[k+1]) in buffer order, row length L, c slots) becomes L
// targets t[T[k]] + i with the slots E[pos[m]] + i in the same order.  Integer
// work only: scans (rocPRIM) and two fill kernels that run one wave per slot /
// per base target, so a 300-entry row is written 64 entries at a time.
#include "pa_internal.h"

#include <cstring>
#include <rocprim/rocprim.hpp>

namespace pa {

// out = exclusive scan of in (n Int64), completed on st
static hipError_t exclusive_sum(const int64_t* in, int64_t* out, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  size_t tb = 0;
  DevBuf<void> tmp;
  hipError_t e = rocprim::exclusive_scan(nullptr, tb, in, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st);
  if (e == hipSuccess) e = tmp.alloc(tb ? tb : 1);
  if (e == hipSuccess) e = rocprim::exclusive_scan(tmp.p, tb, in, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

// ptrs1 (nrows+1, 1-based) checked and written 0-based; *bad |= 1 when the
// first is not 1, |= 2 when they decrease somewhere
__global__ void k_tbl_ptrs(int64_t nrows, const int32_t* __restrict__ ptrs1, int32_t* __restrict__ t,
                           int* __restrict__ bad) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i > nrows) return;
  const int32_t p = ptrs1[i];
  if (i == 0 && p != 1) atomicOr(bad, 1);
  if (i > 0 && p < ptrs1[i - 1]) atomicOr(bad, 2);
  t[i] = p - 1;
}

// len[s] = the row length of slot s's lid for s < n, len[n] = 0 (the scan's total slot)
__global__ void k_tbl_len(int64_t n, const int32_t* __restrict__ lids, const int32_t* __restrict__ t,
                          int64_t* __restrict__ len) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s > n) return;
  int64_t L = 0;
  if (s < n) {
    const int32_t l = lids[s];
    L = (int64_t)t[l + 1] - t[l];
  }
  len[s] = L;
}

// out[j] = E[at[j]] for j < m (the expanded neighbour offsets and the totals)
__global__ void k_tbl_pick(int m, const int64_t* __restrict__ at, const int64_t* __restrict__ E,
                           int64_t* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) out[j] = E[at[j]];
}

// one wave per slot: xl[E[s] + i] = t[l[s]] + i
__global__ void k_tbl_fill(int64_t n, const int32_t* __restrict__ lids, const int32_t* __restrict__ t,
                           const int64_t* __restrict__ E, int32_t* __restrict__ xl) {
  const int64_t s = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (s >= n) return;
  const int32_t l = lids[s];
  const int32_t base = t[l], L = t[l + 1] - base;
  const int64_t e0 = E[s];
  for (int32_t i = lane; i < L; i += 64) xl[e0 + i] = base + i;
}

// per base target k (k < nt): f[k] = its row length, g[k] = row length x its
// slots; f[nt] = g[nt] = 0
__global__ void k_tbl_tlen(int64_t nt, const int32_t* __restrict__ target, const int32_t* __restrict__ ptr,
                           const int32_t* __restrict__ t, int64_t* __restrict__ f, int64_t* __restrict__ g) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k > nt) return;
  int64_t L = 0, c = 0;
  if (k < nt) {
    const int32_t T = target[k];
    L = (int64_t)t[T + 1] - t[T];
    c = ptr[k + 1] - ptr[k];
  }
  f[k] = L;
  g[k] = L * c;
}

// one wave per base target k: its L x c expanded slots, entry i of the row
// major — target F[k] + i = t[T] + i owns xpos[G[k] + i*c .. + c) = E[pos[m]] + i
// for m = ptr[k] .. ptr[k+1]) in that order; the last target closes xptr
__global__ void k_tbl_plan(int64_t nt, const int32_t* __restrict__ target, const int32_t* __restrict__ ptr,
                           const int32_t* __restrict__ pos, const int32_t* __restrict__ t,
                           const int64_t* __restrict__ E, const int64_t* __restrict__ F,
                           const int64_t* __restrict__ G, int32_t* __restrict__ xtarget,
                           int32_t* __restrict__ xptr, int32_t* __restrict__ xpos) {
  const int64_t k = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (k >= nt) return;
  const int32_t T = target[k];
  const int32_t base = t[T];
  const int64_t L = (int64_t)t[T + 1] - base;
  const int32_t p0 = ptr[k];
  const int64_t c = ptr[k + 1] - p0;
  const int64_t f = F[k], g = G[k];
  for (int64_t e = lane; e < L * c; e += 64) {
    const int64_t i = e / c, m = e - i * c;
    xpos[g + e] = (int32_t)(E[pos[p0 + m]] + i);
    if (m == 0) {
      xtarget[f + i] = (int32_t)(base + i);
      xptr[f + i] = (int32_t)(g + e);
    }
  }
  if (k == nt - 1 && lane == 0) xptr[f + L] = (int32_t)(g + L * c);
}

static inline unsigned blocks_for(int64_t threads) { return (unsigned)((threads + 255) / 256); }

// Device ptrs of a new table (pa_table_create with ptrs_on_device): t gets the
// 0-based offsets; *bad as k_tbl_ptrs, *ndata = t[nrows].  Completed on st.
hipError_t table_ptrs(int64_t nrows, const int32_t* d_ptrs1, int32_t* t, int* bad, int64_t* ndata,
                      hipStream_t st) {
  DevBuf<int> dbad;
  hipError_t e = dbad.alloc(1);
  if (e == hipSuccess) e = hipMemsetAsync(dbad.p, 0, sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_tbl_ptrs, dim3(blocks_for(nrows + 1)), dim3(256), 0, st, nrows, d_ptrs1, t, dbad.p);
  e = hipGetLastError();
  int32_t last = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(bad, dbad.p, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&last, t + nrows, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  *ndata = last;
  return e;
}

// One side of a table's derived exchanger from the base side `in` and the
// table offsets t: parts, expanded neighbour offsets, slot count, expanded
// lids, the 16 B-per-slot buffer and the combine plan.  Returns 0; 1 when the
// expanded slots exceed Int32 (*total set, nothing kept); -1 on a HIP error
// (*err).  The host reads back in.parts.size() + 1 offsets and two totals.
// Completed on st when it returns.
int table_expand_side(const XchgSide& in, const int32_t* t, XchgSide* out, int64_t* total, hipStream_t st,
                      hipError_t* err) {
  auto fail = [&](hipError_t e) {
    *err = e;
    return -1;
  };
#define TBL_HIP(expr)                        \
  do {                                       \
    const hipError_t e_ = (expr);            \
    if (e_ != hipSuccess) return fail(e_);   \
  } while (0)
  const int64_t n = in.n;
  out->parts = in.parts;
  out->ptrs.assign(in.ptrs.size(), 0);
  out->n = 0;
  out->plan.unique = true;
  out->plan.ntargets = 0;
  *total = 0;
  if (n == 0) return 0;
  DevBuf<int64_t> len, E, at, picked;
  TBL_HIP(len.alloc(n + 1));
  TBL_HIP(E.alloc(n + 1));
  hipLaunchKernelGGL(k_tbl_len, dim3(blocks_for(n + 1)), dim3(256), 0, st, n, (const int32_t*)in.lids, t, len.p);
  TBL_HIP(hipGetLastError());
  TBL_HIP(exclusive_sum(len.p, E.p, n + 1, st));
  // P'[j] = E[P[j]]; the last base offset is n, so the last picked value is the total
  const int m = (int)in.ptrs.size();
  std::vector<int64_t> got;
  TBL_HIP(at.upload(in.ptrs));
  TBL_HIP(picked.alloc(m));
  hipLaunchKernelGGL(k_tbl_pick, dim3(blocks_for(m)), dim3(256), 0, st, m, (const int64_t*)at.p, (const int64_t*)E.p,
                     picked.p);
  TBL_HIP(hipGetLastError());
  TBL_HIP(download(got, (const int64_t*)picked.p, (size_t)m, st));
  TBL_HIP(hipStreamSynchronize(st));
  *total = got.back();
  if (*total > INT32_MAX) return 1;
  out->ptrs = got;
  out->n = *total;
  out->plan.unique = in.plan.unique;
  out->plan.ntargets = *total;
  if (*total == 0) return 0;
  TBL_HIP(out->lids.alloc(*total));
  TBL_HIP(out->buf.alloc((size_t)*total * 16));
  hipLaunchKernelGGL(k_tbl_fill, dim3(blocks_for(n * 64)), dim3(256), 0, st, n, (const int32_t*)in.lids, t,
                     (const int64_t*)E.p, out->lids.p);
  TBL_HIP(hipGetLastError());
  if (!in.plan.unique) {
    const pa_combine_plan& bp = in.plan;
    const int64_t nt = bp.ntargets;
    DevBuf<int64_t> f, g, F, G;
    TBL_HIP(f.alloc(nt + 1));
    TBL_HIP(g.alloc(nt + 1));
    TBL_HIP(F.alloc(nt + 1));
    TBL_HIP(G.alloc(nt + 1));
    hipLaunchKernelGGL(k_tbl_tlen, dim3(blocks_for(nt + 1)), dim3(256), 0, st, nt, (const int32_t*)bp.d_target,
                       (const int32_t*)bp.d_ptr, t, f.p, g.p);
    TBL_HIP(hipGetLastError());
    TBL_HIP(exclusive_sum(f.p, F.p, nt + 1, st));
    TBL_HIP(exclusive_sum(g.p, G.p, nt + 1, st));
    int64_t ends[2] = {0, 0};  // the expanded targets, and their slots (= the side's total)
    TBL_HIP(hipMemcpyAsync(&ends[0], F.p + nt, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TBL_HIP(hipMemcpyAsync(&ends[1], G.p + nt, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TBL_HIP(hipStreamSynchronize(st));
    if (ends[1] != *total || ends[0] > *total) return fail(hipErrorAssert);  // every slot belongs to one target
    out->plan.ntargets = ends[0];
    TBL_HIP(out->plan.d_target.alloc(ends[0] + 1));
    TBL_HIP(out->plan.d_ptr.alloc(ends[0] + 1));
    TBL_HIP(out->plan.d_pos.alloc(*total));
    hipLaunchKernelGGL(k_tbl_plan, dim3(blocks_for(nt * 64)), dim3(256), 0, st, nt, (const int32_t*)bp.d_target,
                       (const int32_t*)bp.d_ptr, (const int32_t*)bp.d_pos, t, (const int64_t*)E.p,
                       (const int64_t*)F.p, (const int64_t*)G.p, out->plan.d_target.p, out->plan.d_ptr.p,
                       out->plan.d_pos.p);
    TBL_HIP(hipGetLastError());
  }
  TBL_HIP(hipStreamSynchronize(st));
#undef TBL_HIP
  return 0;
}

}  // namespace pa

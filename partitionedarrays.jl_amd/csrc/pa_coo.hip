// pa_coo.hip — `sparse(I, J, V, m, n, +)` and the owned-row SELL build on
// the device (the COO assembly path that feeds A10).
//
// Reference: PSparseMatrix(I,J,V,rows,cols;ids) (Interfaces.jl:2194-2244)
// → compresscoo / sparse (SparseUtils.jl:80-94): duplicates are combined with
// `+` in input order, rows ascend within each column.  Then the SELL layout
// of pa_mat_from_csc: each owned row's entries in the reference's summation
// order (owned columns by oid, then ghost columns by hid; SparseUtils.jl:
// 176-185 over the owned_owned and owned_ghost blocks), ghost rows' stored
// values kept after the SELL slots.
//
// Integer/byte work: two stable radix sorts (rocPRIM) over 64-bit keys, scans
// and scatters.  Duplicate sums run one thread per (i, j) in input order, so
// the result equals the host restatement bit for bit.
#include "pa_internal.h"

#include <cstring>
#include <rocprim/rocprim.hpp>

namespace pa {

// a blocking copy ordered after the work queued on stream st (a plain
// hipMemcpy goes to the null stream, which a non-blocking stream's kernels
// are not ordered against)
static inline hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}


// key = (J-1)*m + (I-1) (column-major = CSC order), or (I-1)*ncols + (J-1)
// (row-major = CSR order, sparsecsr), payload = input position
template <typename IT>
__global__ void k_coo_keys(int64_t n, const IT* __restrict__ I, const IT* __restrict__ J, int64_t m,
                           int64_t ncols, int csr, uint64_t* __restrict__ key, int64_t* __restrict__ idx,
                           int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)I[k] - 1, j = (int64_t)J[k] - 1;
    if (i < 0 || i >= m || j < 0 || j >= ncols) {
      *bad = 1;
      key[k] = 0;
    } else {
      key[k] = csr ? (uint64_t)i * (uint64_t)ncols + (uint64_t)j : (uint64_t)j * (uint64_t)m + (uint64_t)i;
    }
    idx[k] = k;
  }
}

__global__ void k_heads(int64_t n, const uint64_t* __restrict__ key, int64_t* __restrict__ head) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    head[k] = (k == 0 || key[k] != key[k - 1]) ? 1 : 0;
}

// segid = inclusive scan of heads (1-based); start[segid-1] = k at each head
__global__ void k_seg_start(int64_t n, const int64_t* __restrict__ head, const int64_t* __restrict__ segid,
                            int64_t* __restrict__ start) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    if (head[k]) start[segid[k] - 1] = k;
}

// one thread per distinct (i, j): acc = V[first]; acc = acc + V[next] ... in
// input order (the sort is stable)
template <typename T>
__global__ void k_seg_sum(int64_t nu, int64_t n, const int64_t* __restrict__ start, const uint64_t* __restrict__ key,
                          const int64_t* __restrict__ idx, const T* __restrict__ V, int64_t m, int64_t ncols, int csr,
                          int32_t* __restrict__ crow, int32_t* __restrict__ ccol, T* __restrict__ cval) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < nu; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = start[s], b = (s + 1 < nu) ? start[s + 1] : n;
    T acc = V[idx[a]];
    for (int64_t k = a + 1; k < b; ++k) acc = acc + V[idx[k]];
    const uint64_t kk = key[a];
    crow[s] = (int32_t)(csr ? kk / (uint64_t)ncols : kk % (uint64_t)m);
    ccol[s] = (int32_t)(csr ? kk % (uint64_t)ncols : kk / (uint64_t)m);
    cval[s] = acc;
  }
}

// colptr[j] = first nz of column j (lower bound in the column-sorted list);
// for a CSR the same over the rows (ccol = the row of each nz)
__global__ void k_colptr(int64_t ncols, int64_t nu, const int32_t* __restrict__ ccol, int64_t* __restrict__ colptr) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j <= ncols; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = nu;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (ccol[mid] < j) lo = mid + 1; else hi = mid;
    }
    colptr[j] = lo;
  }
}

// owned-row order: key2 = oid*ncols + colpos (colpos = oid of an owned column,
// noids_c + hid of a ghost column); ghost rows sort last (key2 = max)
__global__ void k_own_keys(int64_t nu, const int32_t* __restrict__ crow, const int32_t* __restrict__ ccol,
                           const int32_t* __restrict__ rl2o, const int32_t* __restrict__ cl2o, int64_t noids_c,
                           int64_t ncols, uint64_t* __restrict__ key2, int64_t* __restrict__ idx2,
                           int64_t* __restrict__ gflag) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nu; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t o = rl2o[crow[p]];
    const int32_t oc = cl2o[ccol[p]];
    const int64_t colpos = oc > 0 ? (int64_t)oc - 1 : noids_c + (int64_t)(-oc) - 1;
    key2[p] = o > 0 ? (uint64_t)(o - 1) * (uint64_t)ncols + (uint64_t)colpos : ~0ull;
    idx2[p] = p;
    gflag[p] = o > 0 ? 0 : 1;
  }
}

// rowptr[r] = first owned entry of row r in key2 order
__global__ void k_rowptr(int64_t nrows, int64_t nnz, const uint64_t* __restrict__ key2, int64_t ncols,
                         int64_t* __restrict__ rowptr) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r <= nrows; r += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t target = (uint64_t)r * (uint64_t)ncols;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (key2[mid] < target) lo = mid + 1; else hi = mid;
    }
    rowptr[r] = lo;
  }
}

// per slice: max row length, and whether any row reads a ghost column (its
// last entry, ghost columns sorting after owned ones)
__global__ void k_slice_len(int64_t ns, int64_t nrows, int H, const int64_t* __restrict__ rowptr,
                            const uint64_t* __restrict__ key2, int64_t ncols, int64_t noids_c,
                            const int32_t* __restrict__ lidx, int32_t* __restrict__ slen,
                            int32_t* __restrict__ sghost) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < ns; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r0 = s * H, r1 = (r0 + H < nrows) ? r0 + H : nrows;
    int32_t L = 0, g = 0;
    for (int64_t r = r0; r < r1; ++r) {
      if (lidx && lidx[r] >= 0) continue;  // long rows leave the SELL
      const int64_t a = rowptr[r], b = rowptr[r + 1];
      if (b - a > L) L = (int32_t)(b - a);
      if (b > a && (int64_t)(key2[b - 1] % (uint64_t)ncols) >= noids_c) g = 1;
    }
    slen[s] = L;
    sghost[s] = g;
  }
}

// lidx[r] >= 0: long row r, its entries go to the long CSR at lptr[lidx[r]]
// (values at val[long_off + ..], nz_slot = -(ngh + pos + 1))
template <typename T>
__global__ void k_fill_slots(int64_t nnz, const uint64_t* __restrict__ key2, const int64_t* __restrict__ idx2,
                             const int64_t* __restrict__ rowptr, const int64_t* __restrict__ soff, int H, int R,
                             int64_t ncols, const int32_t* __restrict__ ccol, const T* __restrict__ cval,
                             int32_t* __restrict__ col, T* __restrict__ val, int64_t* __restrict__ nz_slot,
                             const int32_t* __restrict__ lidx, const int64_t* __restrict__ lptr,
                             int32_t* __restrict__ lcol, int64_t long_off, int64_t ngh) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = (int64_t)(key2[t] / (uint64_t)ncols);
    const int64_t k = t - rowptr[r];
    if (lidx && lidx[r] >= 0) {
      const int64_t pos = lptr[lidx[r]] + k;
      const int64_t p = idx2[t];
      lcol[pos] = ccol[p];
      val[long_off + pos] = cval[p];
      nz_slot[p] = -(ngh + pos + 1);
      continue;
    }
    const int64_t s = r / H, w = r - s * H;
    const int64_t slot = soff[s] + (k * 64 + w / R) * R + (w % R);
    const int64_t p = idx2[t];
    col[slot] = ccol[p];
    val[slot] = cval[p];
    nz_slot[p] = slot;
  }
}

// ghost-row nonzeros in CSC order after the slots: nz_slot = -(rank+1);
// grc keeps their (row lid, col lid) for the entry views (pa_mat::d_ghost_rc)
template <typename T>
__global__ void k_fill_ghost(int64_t nu, const int64_t* __restrict__ gflag, const int64_t* __restrict__ grank,
                             const T* __restrict__ cval, int64_t slots, T* __restrict__ val,
                             int64_t* __restrict__ nz_slot, const int32_t* __restrict__ crow,
                             const int32_t* __restrict__ ccol, int32_t* __restrict__ grc) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < nu; p += (int64_t)gridDim.x * blockDim.x)
    if (gflag[p]) {
      const int64_t g = grank[p];
      nz_slot[p] = -(g + 1);
      val[slots + g] = cval[p];
      grc[2 * g] = crow[p];
      grc[2 * g + 1] = ccol[p];
    }
}

__global__ void k_fill_i32(int64_t n, int32_t* __restrict__ a, int32_t v) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    a[k] = v;
}

namespace {

inline dim3 grid1(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g < 1) g = 1;
  if (g > 16384) g = 16384;
  return dim3((unsigned)g);
}

inline int bits_for(uint64_t maxkey) {
  int b = 1;
  while (b < 64 && (maxkey >> b)) ++b;
  return b;
}

// stable sort of (key, idx) pairs in place (double buffer + temp storage);
// 64-bit keys and payloads, or 32-bit ones (the ordered vector scatter)
template <typename K, typename P>
hipError_t sort_pairs(DevBuf<K>& key, DevBuf<P>& idx, int64_t n, int end_bit, hipStream_t st) {
  if (n <= 1) return hipSuccess;
  DevBuf<K> k2;
  DevBuf<P> i2;
  DevBuf<void> tmp;
  size_t tb = 0;
  hipError_t e = k2.alloc(n);
  if (e == hipSuccess) e = i2.alloc(n);
  rocprim::double_buffer<K> kb(key.p, k2.p);
  rocprim::double_buffer<P> ib(idx.p, i2.p);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(nullptr, tb, kb, ib, (size_t)n, 0, (unsigned)end_bit, st);
  if (e == hipSuccess) e = tmp.alloc(tb ? tb : 1);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs(tmp.p, tb, kb, ib, (size_t)n, 0, (unsigned)end_bit, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  // keep the buffers holding the result
  if (kb.current() != key.p) std::swap(key.p, k2.p);
  if (ib.current() != idx.p) std::swap(idx.p, i2.p);
  return e;
}

hipError_t inclusive_sum(const int64_t* in, int64_t* out, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  size_t tb = 0;
  DevBuf<void> tmp;
  hipError_t e = rocprim::inclusive_scan(nullptr, tb, in, out, (size_t)n, rocprim::plus<int64_t>(), st);
  if (e == hipSuccess) e = tmp.alloc(tb ? tb : 1);
  if (e == hipSuccess) e = rocprim::inclusive_scan(tmp.p, tb, in, out, (size_t)n, rocprim::plus<int64_t>(), st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

hipError_t exclusive_sum(const int64_t* in, int64_t* out, int64_t n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  size_t tb = 0;
  DevBuf<void> tmp;
  hipError_t e = rocprim::exclusive_scan(nullptr, tb, in, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st);
  if (e == hipSuccess) e = tmp.alloc(tb ? tb : 1);
  if (e == hipSuccess) e = rocprim::exclusive_scan(tmp.p, tb, in, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

// rank = exclusive scan of the 0/1 flags; *count = the flagged items (the
// last rank + the last flag, read back)
hipError_t scan_count(const int64_t* flag, int64_t* rank, int64_t n, hipStream_t st, int64_t* count) {
  int64_t last[2] = {0, 0};
  *count = 0;
  if (n <= 0) return hipSuccess;
  hipError_t e = exclusive_sum(flag, rank, n, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&last[0], rank + n - 1, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&last[1], flag + n - 1, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  *count = last[0] + last[1];
  return e;
}

template <typename T>
void seg_sum_t(int64_t nu, int64_t n, const int64_t* start, const uint64_t* key, const int64_t* idx,
               const void* V, int64_t m, int64_t ncols, int csr, int32_t* crow, int32_t* ccol, void* cval,
               hipStream_t st) {
  hipLaunchKernelGGL(k_seg_sum<T>, grid1(nu), dim3(256), 0, st, nu, n, start, key, idx, (const T*)V, m, ncols, csr,
                     crow, ccol, (T*)cval);
}

}  // namespace

// leave the function with `ret` when a HIP call fails (the DevBuf locals
// and the caller's outputs release what was allocated so far)
#define PA_HIP_OR(expr, ret)             \
  do {                                   \
    if ((expr) != hipSuccess) return ret; \
  } while (0)

// Phase A: sparse(I, J, V, m, n, +) → CSC on the device (0-based rows/cols,
// values combined).  I, J: 1-based device arrays (index_bytes 4 or 8).
// Outputs: crow, ccol, cval (nu entries) and colptr (ncols+1, 0-based
// offsets).  Returns 1 on an out-of-range index, -1 on a HIP error (*err).
// csr: sparsecsr instead — the nonzeros in row-major (CSR) order and
// colptr the row pointers (m+1).
int coo_compress(int dtype, int index_bytes, int64_t m, int64_t ncols, int64_t n, const void* dI, const void* dJ,
                 const void* dV, int csr, int64_t* nu_out, DevBuf<int32_t>& crow, DevBuf<int32_t>& ccol,
                 DevBuf<void>& cval, DevBuf<int64_t>& colptr, hipStream_t st, hipError_t* err) {
  const size_t S = dtype_size(dtype);
  DevBuf<uint64_t> key;
  DevBuf<int64_t> idx, head, segid, start;
  DevBuf<int> bad;
  int hbad = 0;
  int64_t nu = 0;
  *nu_out = 0;
  *err = hipSuccess;
  const int64_t nptr = csr ? m : ncols;  // columns (CSC) or rows (CSR) of the compressed axis
  PA_HIP_OR(*err = colptr.alloc(nptr + 1), -1);
  if (n > 0) {
    PA_HIP_OR(*err = key.alloc(n), -1);
    PA_HIP_OR(*err = idx.alloc(n), -1);
    PA_HIP_OR(*err = bad.alloc(1), -1);
    PA_HIP_OR(*err = hipMemsetAsync(bad, 0, sizeof(int), st), -1);
    if (index_bytes == 8)
      hipLaunchKernelGGL(k_coo_keys<int64_t>, grid1(n), dim3(256), 0, st, n, (const int64_t*)dI, (const int64_t*)dJ,
                         m, ncols, csr, key.p, idx.p, bad.p);
    else
      hipLaunchKernelGGL(k_coo_keys<int32_t>, grid1(n), dim3(256), 0, st, n, (const int32_t*)dI, (const int32_t*)dJ,
                         m, ncols, csr, key.p, idx.p, bad.p);
    PA_HIP_OR(*err = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st), -1);
    PA_HIP_OR(*err = hipStreamSynchronize(st), -1);
    if (hbad) return 1;
    PA_HIP_OR(*err = sort_pairs(key, idx, n, bits_for((uint64_t)m * (uint64_t)ncols), st), -1);
    PA_HIP_OR(*err = head.alloc(n), -1);
    PA_HIP_OR(*err = segid.alloc(n), -1);
    hipLaunchKernelGGL(k_heads, grid1(n), dim3(256), 0, st, n, key.p, head.p);
    PA_HIP_OR(*err = inclusive_sum(head, segid, n, st), -1);
    PA_HIP_OR(*err = copy_sync(&nu, segid.p + n - 1, 8, hipMemcpyDeviceToHost, st), -1);
    PA_HIP_OR(*err = start.alloc(nu), -1);
    hipLaunchKernelGGL(k_seg_start, grid1(n), dim3(256), 0, st, n, head.p, segid.p, start.p);
    PA_HIP_OR(*err = crow.alloc(nu), -1);
    PA_HIP_OR(*err = ccol.alloc(nu), -1);
    PA_HIP_OR(*err = cval.alloc(nu * S), -1);
    switch (dtype) {
      case PA_F32: seg_sum_t<float>(nu, n, start, key, idx, dV, m, ncols, csr, crow, ccol, cval, st); break;
      case PA_F64: seg_sum_t<double>(nu, n, start, key, idx, dV, m, ncols, csr, crow, ccol, cval, st); break;
      case PA_C64: seg_sum_t<c64>(nu, n, start, key, idx, dV, m, ncols, csr, crow, ccol, cval, st); break;
      case PA_C128: seg_sum_t<c128>(nu, n, start, key, idx, dV, m, ncols, csr, crow, ccol, cval, st); break;
    }
  }
  hipLaunchKernelGGL(k_colptr, grid1(nptr + 1), dim3(256), 0, st, nptr, nu, csr ? crow.p : ccol.p, colptr.p);
  PA_HIP_OR(*err = hipGetLastError(), -1);
  PA_HIP_OR(*err = hipStreamSynchronize(st), -1);
  *nu_out = nu;
  return 0;
}

// Phase B, first half: order the owned rows' entries (key2/idx2, nnz owned
// entries first), row pointers, per-slice lengths / ghost flags, ghost-row
// flags and ranks.
int coo_row_order(int64_t nu, const int32_t* crow, const int32_t* ccol, const int32_t* rl2o, const int32_t* cl2o,
                  int64_t nrows, int64_t noids_c, int64_t ncols, int H, DevBuf<uint64_t>& key2, DevBuf<int64_t>& idx2,
                  DevBuf<int64_t>& rowptr, DevBuf<int64_t>& gflag, DevBuf<int64_t>& grank, DevBuf<int32_t>& slen,
                  DevBuf<int32_t>& sghost, int64_t* nnz_out, int64_t* ngh_out, hipStream_t st, hipError_t* err) {
  const int64_t ns = (nrows + H - 1) / H;
  int64_t nnz = 0, ngh = 0;
  *nnz_out = *ngh_out = 0;
  *err = hipSuccess;
  const int64_t nb = nu > 0 ? nu : 1;
  PA_HIP_OR(*err = key2.alloc(nb), -1);
  PA_HIP_OR(*err = idx2.alloc(nb), -1);
  PA_HIP_OR(*err = gflag.alloc(nb), -1);
  PA_HIP_OR(*err = grank.alloc(nb), -1);
  PA_HIP_OR(*err = rowptr.alloc(nrows + 1), -1);
  PA_HIP_OR(*err = slen.alloc(ns > 0 ? ns : 1), -1);
  PA_HIP_OR(*err = sghost.alloc(ns > 0 ? ns : 1), -1);
  if (nu > 0) {
    hipLaunchKernelGGL(k_own_keys, grid1(nu), dim3(256), 0, st, nu, crow, ccol, rl2o, cl2o, noids_c, ncols, key2.p,
                       idx2.p, gflag.p);
    PA_HIP_OR(*err = scan_count(gflag, grank, nu, st, &ngh), -1);
    nnz = nu - ngh;
    // ghost rows carry key2 = ~0: sort all bits of the owned range + 1
    const uint64_t maxk = (uint64_t)(nrows > 0 ? nrows : 1) * (uint64_t)ncols;
    PA_HIP_OR(*err = sort_pairs(key2, idx2, nu, ngh ? 64 : bits_for(maxk), st), -1);
  }
  hipLaunchKernelGGL(k_rowptr, grid1(nrows + 1), dim3(256), 0, st, nrows, nnz, key2.p, ncols, rowptr.p);
  PA_HIP_OR(*err = hipGetLastError(), -1);
  PA_HIP_OR(*err = hipStreamSynchronize(st), -1);
  *nnz_out = nnz;
  *ngh_out = ngh;
  return 0;
}

// Phase B, second half: scatter into the SELL slots (col pre-filled with -1,
// val zeroed by the caller) and the ghost-row values after them.
// per-slice max row length and ghost flag of the SELL rows (long rows skipped)
void coo_slices(int64_t ns, int64_t nrows, int H, const int64_t* rowptr, const uint64_t* key2, int64_t ncols,
                int64_t noids_c, const int32_t* lidx, int32_t* slen, int32_t* sghost, hipStream_t st) {
  if (ns > 0)
    hipLaunchKernelGGL(k_slice_len, grid1(ns), dim3(256), 0, st, ns, nrows, H, rowptr, key2, ncols, noids_c, lidx,
                       slen, sghost);
}

void coo_fill(int dtype, int64_t nnz, int64_t nu, const uint64_t* key2, const int64_t* idx2, const int64_t* rowptr,
              const int64_t* soff, int H, int R, int64_t ncols, const int32_t* crow, const int32_t* ccol,
              const void* cval, const int64_t* gflag, const int64_t* grank, int64_t slots, int32_t* col, void* val,
              int64_t* nz_slot, const int32_t* lidx, const int64_t* lptr, int32_t* lcol, int64_t long_off,
              int32_t* grc, hipStream_t st) {
  const int64_t ngh = long_off - slots;
#define PA_FILL(T)                                                                                             \
  if (nnz > 0)                                                                                                 \
    hipLaunchKernelGGL(k_fill_slots<T>, grid1(nnz), dim3(256), 0, st, nnz, key2, idx2, rowptr, soff, H, R,     \
                       ncols, ccol, (const T*)cval, col, (T*)val, nz_slot, lidx, lptr, lcol, long_off, ngh);   \
  if (nu > 0 && ngh > 0)                                                                                       \
    hipLaunchKernelGGL(k_fill_ghost<T>, grid1(nu), dim3(256), 0, st, nu, gflag, grank, (const T*)cval, slots, \
                       (T*)val, nz_slot, crow, ccol, grc);
  switch (dtype) {
    case PA_F32: { PA_FILL(float) } break;
    case PA_F64: { PA_FILL(double) } break;
    case PA_C64: { PA_FILL(c64) } break;
    case PA_C128: { PA_FILL(c128) } break;
  }
#undef PA_FILL
}

void launch_fill_i32(int64_t n, int32_t* a, int32_t v, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_fill_i32, grid1(n), dim3(256), 0, st, n, a, v);
}

}  // namespace pa

// ---------------------------------------------------------------------------
// Global ids on the device: the gid → lid table of an
// index set (sorted gids + their lids), `to_lids!` (Interfaces.jl:1541-1543)
// and the first-touch ghost discovery of `add_gids!` (579-603, 1515-1533).

namespace pa {

__global__ void k_iota_i64(int64_t n, int64_t* __restrict__ a) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    a[k] = k;
}

// lid (0-based) of gid, or -1: binary search in the sorted gid table
__device__ inline int64_t gid_lookup(int64_t g, const uint64_t* __restrict__ sgid, const int64_t* __restrict__ slid,
                                     int64_t nl) {
  int64_t lo = 0, hi = nl;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)sgid[mid] < g) lo = mid + 1; else hi = mid;
  }
  return (lo < nl && (int64_t)sgid[lo] == g) ? slid[lo] : -1;
}

// ids (1-based gids) → 1-based lids in place; *bad = 1 if a gid is absent
__global__ void k_to_lids(int64_t n, int64_t* __restrict__ ids, const uint64_t* __restrict__ sgid,
                          const int64_t* __restrict__ slid, int64_t nl, int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = gid_lookup(ids[k], sgid, slid, nl);
    if (l < 0) *bad = 1;
    ids[k] = l + 1;
  }
}

// flag[k] = gid absent from the table
__global__ void k_absent(int64_t n, const int64_t* __restrict__ gids, const uint64_t* __restrict__ sgid,
                         const int64_t* __restrict__ slid, int64_t nl, int64_t* __restrict__ flag) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    flag[k] = gid_lookup(gids[k], sgid, slid, nl) < 0 ? 1 : 0;
}

__global__ void k_compact(int64_t n, const int64_t* __restrict__ gids, const int64_t* __restrict__ flag,
                          const int64_t* __restrict__ pos, uint64_t* __restrict__ key, int64_t* __restrict__ val) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    if (flag[k]) {
      key[pos[k]] = (uint64_t)gids[k];
      val[pos[k]] = k;
    }
}

// after sorting (gid, position) pairs: at each distinct gid, its first
// position becomes the key and the gid the payload
__global__ void k_first_touch(int64_t m, const uint64_t* __restrict__ key, const int64_t* __restrict__ val,
                              const int64_t* __restrict__ head, const int64_t* __restrict__ rank,
                              uint64_t* __restrict__ key2, int64_t* __restrict__ val2) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x)
    if (head[k]) {
      key2[rank[k] - 1] = (uint64_t)val[k];
      val2[rank[k] - 1] = (int64_t)key[k];
    }
}

// the largest of n device values (it bounds the radix passes of a gid sort)
static hipError_t device_max(const int64_t* in, int64_t n, int64_t* out, hipStream_t st) {
  size_t tb = 0;
  DevBuf<void> tmp;
  DevBuf<int64_t> dmax;
  hipError_t e = dmax.alloc(1);
  if (e == hipSuccess) e = rocprim::reduce(nullptr, tb, in, dmax.p, (int64_t)0, (size_t)n, rocprim::maximum<int64_t>(), st);
  if (e == hipSuccess) e = tmp.alloc(tb ? tb : 1);
  if (e == hipSuccess) e = rocprim::reduce(tmp.p, tb, in, dmax.p, (int64_t)0, (size_t)n, rocprim::maximum<int64_t>(), st);
  if (e == hipSuccess) e = hipMemcpyAsync(out, dmax, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

// sorted (gid, lid) table of lid_to_gid (device input, n lids)
int gid_table(int64_t n, const int64_t* d_lid_to_gid, DevBuf<uint64_t>& sgid, DevBuf<int64_t>& slid, hipStream_t st) {
  sgid.reset();
  slid.reset();
  if (n <= 0) return 0;
  int64_t maxg = 0;
  PA_HIP_OR(sgid.alloc(n), -1);
  PA_HIP_OR(slid.alloc(n), -1);
  PA_HIP_OR(hipMemcpyAsync(sgid, d_lid_to_gid, n * 8, hipMemcpyDeviceToDevice, st), -1);
  hipLaunchKernelGGL(k_iota_i64, grid1(n), dim3(256), 0, st, n, slid.p);
  PA_HIP_OR(device_max(d_lid_to_gid, n, &maxg, st), -1);
  PA_HIP_OR(sort_pairs(sgid, slid, n, bits_for((uint64_t)(maxg > 0 ? maxg : 1)), st), -1);
  return 0;
}

// ids (n, device, 1-based gids) → 1-based lids; returns 1 if a gid is absent
int gids_to_lids(int64_t n, int64_t* ids, const uint64_t* sgid, const int64_t* slid, int64_t nl, hipStream_t st) {
  if (n <= 0) return 0;
  DevBuf<int> bad;
  int hbad = 0;
  PA_HIP_OR(bad.alloc(1), -1);
  hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), st);
  hipLaunchKernelGGL(k_to_lids, grid1(n), dim3(256), 0, st, n, ids, sgid, slid, nl, bad.p);
  if (e == hipSuccess) e = hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return -1;
  return hbad ? 1 : 0;
}

// ids (1-based lids) → 1-based gids in place through lid_to_gid (nl entries);
// *bad = 1 if a lid is outside 1..nl (that id is left as it was)
__global__ void k_to_gids(int64_t n, int64_t* __restrict__ ids, const int64_t* __restrict__ l2g, int64_t nl,
                          int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = ids[k];
    if (l < 1 || l > nl) *bad = 1;
    else ids[k] = l2g[l - 1];
  }
}

// ids (n, device, 1-based lids) → 1-based gids; returns 1 if a lid is out of range
int lids_to_gids(int64_t n, int64_t* ids, const int64_t* l2g, int64_t nl, hipStream_t st) {
  if (n <= 0) return 0;
  DevBuf<int> bad;
  int hbad = 0;
  PA_HIP_OR(bad.alloc(1), -1);
  PA_HIP_OR(hipMemsetAsync(bad, 0, sizeof(int), st), -1);
  hipLaunchKernelGGL(k_to_gids, grid1(n), dim3(256), 0, st, n, ids, l2g, nl, bad.p);
  PA_HIP_OR(hipGetLastError(), -1);
  PA_HIP_OR(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);
  return hbad ? 1 : 0;
}

// add_gids!: the gids (device, n) absent from the table, each once, in order
// of first occurrence: out (device, *m_out entries)
int gids_first_touch(int64_t n, const int64_t* gids, const uint64_t* sgid, const int64_t* slid, int64_t nl,
                     DevBuf<int64_t>& out, int64_t* m_out, hipStream_t st) {
  out.reset();
  *m_out = 0;
  if (n <= 0) return 0;
  DevBuf<int64_t> flag, pos, val, head, rank, val2;
  DevBuf<uint64_t> key, key2;
  int64_t m = 0, u = 0, maxg = 0;
  PA_HIP_OR(flag.alloc(n), -1);
  PA_HIP_OR(pos.alloc(n), -1);
  hipLaunchKernelGGL(k_absent, grid1(n), dim3(256), 0, st, n, gids, sgid, slid, nl, flag.p);
  PA_HIP_OR(scan_count(flag, pos, n, st, &m), -1);
  if (m == 0) return 0;
  PA_HIP_OR(key.alloc(m), -1);
  PA_HIP_OR(val.alloc(m), -1);
  hipLaunchKernelGGL(k_compact, grid1(n), dim3(256), 0, st, n, gids, flag.p, pos.p, key.p, val.p);
  flag.reset();
  pos.reset();
  PA_HIP_OR(device_max((const int64_t*)key.p, m, &maxg, st), -1);
  PA_HIP_OR(sort_pairs(key, val, m, bits_for((uint64_t)(maxg > 0 ? maxg : 1)), st), -1);
  PA_HIP_OR(head.alloc(m), -1);
  PA_HIP_OR(rank.alloc(m), -1);
  hipLaunchKernelGGL(k_heads, grid1(m), dim3(256), 0, st, m, key.p, head.p);
  PA_HIP_OR(inclusive_sum(head, rank, m, st), -1);
  PA_HIP_OR(copy_sync(&u, rank.p + m - 1, 8, hipMemcpyDeviceToHost, st), -1);
  PA_HIP_OR(key2.alloc(u), -1);
  PA_HIP_OR(val2.alloc(u), -1);
  hipLaunchKernelGGL(k_first_touch, grid1(m), dim3(256), 0, st, m, key.p, val.p, head.p, rank.p, key2.p, val2.p);
  PA_HIP_OR(sort_pairs(key2, val2, u, bits_for((uint64_t)n), st), -1);
  out = std::move(val2);
  *m_out = u;
  return 0;
}

// ---------------------------------------------------------------------------
// async_assemble!(I, J, V, rows) (Interfaces.jl:2406-2492) on the device: the
// triplets whose row is owned by another part are grouped by owner (segments
// in rows.exchanger.parts_rcv order, input order inside each), copied out
// and their local value set to zero; the host side (pa_api.cpp) moves the
// segments to the owners, which append them in parts_snd order.

// seg_of_lid[lids_rcv[t]] = the segment of slot t (every ghost lid is in
// exactly one receive segment: the one of its owner, Interfaces.jl:740-762)
__global__ void k_seg_of_lid(int64_t nslots, const int32_t* __restrict__ lids_rcv, const int64_t* __restrict__ ptrs,
                             int nseg, int32_t* __restrict__ seg_of_lid) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nslots; t += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nseg;  // last segment whose start <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (ptrs[mid] <= t) lo = mid; else hi = mid;
    }
    seg_of_lid[lids_rcv[t]] = lo;
  }
}

// key[k] = 0 for a row owned here, 1 + segment of the row's owner otherwise
// (rows' gid table: an absent gid is the KeyError of to_lids!; a ghost row
// that no receive segment lists is the KeyError of owner_to_i,
// Interfaces.jl:2428-2430: the exchanger does not match the rows)
__global__ void k_coo_seg(int64_t n, const int64_t* __restrict__ I, const uint64_t* __restrict__ sgid,
                          const int64_t* __restrict__ slid, int64_t nl, const int32_t* __restrict__ seg_of_lid,
                          uint64_t* __restrict__ key, int64_t* __restrict__ idx, int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = gid_lookup(I[k], sgid, slid, nl);
    const int32_t sg = l < 0 ? -1 : seg_of_lid[l];
    if (l < 0) *bad = 1;
    else if (sg == -2) *bad = 2;  // a ghost row whose owner is not in parts_rcv
    key[k] = sg < 0 ? 0 : (uint64_t)(sg + 1);
    idx[k] = k;
  }
}

// first[key] = the first position of each key of the sorted keys
__global__ void k_key_first(int64_t n, const uint64_t* __restrict__ key, int64_t* __restrict__ first) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
    if (t == 0 || key[t] != key[t - 1]) first[key[t]] = t;
}

// the nr sent triplets in segment order: sI/sJ/sV[t] = I/J/V[idx[t]]; with
// ZERO_SRC (assemble!) the local value becomes zero(v) (the entry stays in
// the local list), without it (exchange!) the local entry is left as it is
template <typename T, bool ZERO_SRC>
__global__ void k_coo_pack(int64_t nr, const int64_t* __restrict__ idx, const int64_t* __restrict__ I,
                           const int64_t* __restrict__ J, T* __restrict__ V, int64_t* __restrict__ sI,
                           int64_t* __restrict__ sJ, T* __restrict__ sV) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nr; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = idx[t];
    sI[t] = I[k];
    sJ[t] = J[k];
    sV[t] = V[k];
    if (ZERO_SRC) V[k] = zero_of<T>();
  }
}

template <typename T>
static void coo_pack_t(int64_t nr, const int64_t* idx, const int64_t* I, const int64_t* J, void* V, bool zero_src,
                       int64_t* sI, int64_t* sJ, void* sV, hipStream_t st) {
  auto kern = zero_src ? k_coo_pack<T, true> : k_coo_pack<T, false>;
  hipLaunchKernelGGL(kern, grid1(nr), dim3(256), 0, st, nr, idx, I, J, (T*)V, sI, sJ, (T*)sV);
}

// The common tail of the two send sides: key[k] = 0 (stays) or 1 + segment,
// idx[k] = k.  Sorts by key (stable: input order inside a segment), counts
// the segments into cnt[0..nseg) and copies the sent triplets out, segment
// after segment, into *out.
static hipError_t coo_pack_by_key(int dtype, const CooList& in, DevBuf<uint64_t>& key, DevBuf<int64_t>& idx, int nseg,
                                  bool zero_src, CooList* out, std::vector<int64_t>* cnt, hipStream_t st) {
  const size_t S = dtype_size(dtype);
  const int64_t n = in.n;
  DevBuf<int64_t> first;
  std::vector<int64_t> hfirst(nseg + 2, -1);
  hipError_t e = sort_pairs(key, idx, n, bits_for((uint64_t)nseg + 1), st);
  if (e == hipSuccess) e = first.alloc(nseg + 2);
  if (e == hipSuccess) e = hipMemsetAsync(first, 0xff, (nseg + 2) * 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_key_first, grid1(n), dim3(256), 0, st, n, key.p, first.p);
  e = hipMemcpyAsync(hfirst.data(), first, (nseg + 1) * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  // end of key q = start of the next present key, or n
  hfirst[nseg + 1] = n;
  std::vector<int64_t> start(nseg + 2, n);
  for (int q = nseg; q >= 0; --q) start[q] = hfirst[q] >= 0 ? hfirst[q] : start[q + 1];
  const int64_t nloc = start[1], nr = n - nloc;
  for (int q = 0; q < nseg; ++q) (*cnt)[q] = start[q + 2] - start[q + 1];
  if (nr > 0) {
    e = out->I.alloc(nr);
    if (e == hipSuccess) e = out->J.alloc(nr);
    if (e == hipSuccess) e = out->V.alloc(nr * S);
    if (e != hipSuccess) return e;
    out->n = nr;
    switch (dtype) {
      case PA_F32: coo_pack_t<float>(nr, idx.p + nloc, in.I, in.J, in.V, zero_src, out->I, out->J, out->V, st); break;
      case PA_F64: coo_pack_t<double>(nr, idx.p + nloc, in.I, in.J, in.V, zero_src, out->I, out->J, out->V, st); break;
      case PA_C64: coo_pack_t<c64>(nr, idx.p + nloc, in.I, in.J, in.V, zero_src, out->I, out->J, out->V, st); break;
      case PA_C128: coo_pack_t<c128>(nr, idx.p + nloc, in.I, in.J, in.V, zero_src, out->I, out->J, out->V, st); break;
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  return e;
}

// ---------------------------------------------------------------------------
// async_exchange!(I, J, V, rows) (Interfaces.jl:2494-2592) on the device, the
// mirror of the assembly above: the triplets of the rows that other parts
// hold as ghosts are copied out per neighbour (segments in
// rows.exchanger.parts_snd order, input order inside each) and stay in the
// local list unchanged; the host side (pa_api.cpp) moves the segments to the
// ghost holders, which append them in parts_rcv order.

// snd_of_lid[l] (0 for an owned lid, -1 for a ghost lid on entry) becomes
// 1 + the last segment of lids_snd that lists l: the reference's loop
// `lid_to_i[lid] = i` (2514-2520) overwrites, so a lid that several
// neighbours hold as a ghost keeps the last of them.  Slots of different
// segments may name the same lid, hence the atomic max and not a store.
__global__ void k_snd_seg_of_lid(int64_t nslots, const int32_t* __restrict__ lids_snd,
                                 const int64_t* __restrict__ ptrs, int nseg, int32_t* __restrict__ snd_of_lid) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nslots; t += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nseg;  // last segment whose start <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (ptrs[mid] <= t) lo = mid; else hi = mid;
    }
    atomicMax(&snd_of_lid[lids_snd[t]], lo + 1);
  }
}

// key[k] = 1 + the send segment of the row's lid, or 0 when no neighbour
// holds the row; then a ghost row's value becomes zero(Tv) (2529-2530: an
// exact +0, not v*0) and an owned row's triplet is left alone.  *bad = 1 for
// a row gid that is not a local id of rows (the KeyError of to_lids!).
template <typename T>
__global__ void k_coo_xseg(int64_t n, const int64_t* __restrict__ I, T* __restrict__ V,
                           const uint64_t* __restrict__ sgid, const int64_t* __restrict__ slid, int64_t nl,
                           const int32_t* __restrict__ snd_of_lid, uint64_t* __restrict__ key,
                           int64_t* __restrict__ idx, int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = gid_lookup(I[k], sgid, slid, nl);
    const int32_t sg = l < 0 ? 0 : snd_of_lid[l];
    if (l < 0) *bad = 1;
    else if (sg < 0) V[k] = zero_of<T>();
    key[k] = sg > 0 ? (uint64_t)sg : 0;
    idx[k] = k;
  }
}

template <typename T>
static void coo_xseg_t(int64_t n, const int64_t* I, void* V, const uint64_t* sgid, const int64_t* slid, int64_t nl,
                       const int32_t* snd_of_lid, uint64_t* key, int64_t* idx, int* bad, hipStream_t st) {
  hipLaunchKernelGGL(k_coo_xseg<T>, grid1(n), dim3(256), 0, st, n, I, (T*)V, sgid, slid, nl, snd_of_lid, key, idx,
                     bad);
}

// One part's send side of assemble! (to_ghosts = false, side = the
// exchanger's rcv list: the triplets of the ghost rows go to the rows'
// owners and become zero here) or exchange! (to_ghosts = true, side = its
// snd list: the triplets of the rows that neighbours hold as ghosts).
// Outputs: *out (the sent triplets, segment after segment) and
// cnt[0..nseg) on the host, nseg = the side's neighbours.  Every lid of the
// side is below nl (checked by the caller).  Returns 1 when a row gid is not
// a local id of rows (KeyError; exchange!: ghost rows met before that may
// already hold zero, as the reference leaves I half converted), 2 when a
// ghost row's owner has no receive segment (assemble!, KeyError).
int coo_send_pack(bool to_ghosts, int dtype, const CooList& in, const uint64_t* sgid, const int64_t* slid, int64_t nl,
                  const std::vector<int32_t>& lid_to_ohid, const XchgSide& side, CooList* out,
                  std::vector<int64_t>* cnt, hipStream_t st) {
  const int nseg = (int)side.parts.size();
  const int64_t n = in.n;
  *out = CooList{};
  cnt->assign(nseg, 0);
  if (n <= 0) return 0;
  DevBuf<int32_t> sol;
  DevBuf<int64_t> dptrs, idx;
  DevBuf<uint64_t> key;
  DevBuf<int> bad;
  int hbad = 0;
  const int64_t nslots = side.ptrs.empty() ? 0 : side.ptrs.back();
  // a lid's mark before the side's slots are visited.  assemble!: -1 owned,
  // -2 ghost (k_seg_of_lid then sets its segment); exchange!: 0 owned, -1
  // ghost (k_snd_seg_of_lid then raises the listed ones)
  const int32_t owned = to_ghosts ? 0 : -1, ghost = owned - 1;
  std::vector<int32_t> hs(nl > 0 ? nl : 1, owned);
  for (int64_t l = 0; l < nl; ++l) hs[l] = lid_to_ohid[l] > 0 ? owned : ghost;
  PA_HIP_OR(sol.alloc(hs.size()), -1);
  PA_HIP_OR(copy_sync(sol, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, st), -1);
  if (nslots > 0) {
    PA_HIP_OR(dptrs.alloc(side.ptrs.size()), -1);
    PA_HIP_OR(hipMemcpyAsync(dptrs, side.ptrs.data(), side.ptrs.size() * 8, hipMemcpyHostToDevice, st), -1);
    if (to_ghosts)
      hipLaunchKernelGGL(k_snd_seg_of_lid, grid1(nslots), dim3(256), 0, st, nslots, side.lids.p, dptrs.p, nseg, sol.p);
    else
      hipLaunchKernelGGL(k_seg_of_lid, grid1(nslots), dim3(256), 0, st, nslots, side.lids.p, dptrs.p, nseg, sol.p);
  }
  PA_HIP_OR(key.alloc(n), -1);
  PA_HIP_OR(idx.alloc(n), -1);
  PA_HIP_OR(bad.alloc(1), -1);
  PA_HIP_OR(hipMemsetAsync(bad, 0, sizeof(int), st), -1);
  if (!to_ghosts) {
    hipLaunchKernelGGL(k_coo_seg, grid1(n), dim3(256), 0, st, n, in.I.p, sgid, slid, nl, sol.p, key.p, idx.p, bad.p);
  } else {
    switch (dtype) {
      case PA_F32: coo_xseg_t<float>(n, in.I, in.V, sgid, slid, nl, sol, key, idx, bad, st); break;
      case PA_F64: coo_xseg_t<double>(n, in.I, in.V, sgid, slid, nl, sol, key, idx, bad, st); break;
      case PA_C64: coo_xseg_t<c64>(n, in.I, in.V, sgid, slid, nl, sol, key, idx, bad, st); break;
      case PA_C128: coo_xseg_t<c128>(n, in.I, in.V, sgid, slid, nl, sol, key, idx, bad, st); break;
    }
  }
  PA_HIP_OR(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);
  if (hbad) return hbad;  // 1: unknown gid, 2: ghost row without a segment (assemble! only)
  return coo_pack_by_key(dtype, in, key, idx, nseg, !to_ghosts, out, cnt, st) == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// PVector(I, V, rows; ids) (Interfaces.jl:1887-1932) and the writes and reads
// of local_view / global_view (1994-2069) on the device: an ordered scatter
// of n pairs (id, V) into one part's values, and its gather twin.  The
// reference's loop `values[lid] += V[i]` runs in input order; here the pairs
// are sorted stably by lid (input position as payload) and the thread at the
// first entry of each distinct lid folds that lid's entries in input order
// with plain adds, so the result equals the loop's bit for bit whatever the
// duplicates, without atomics.

// the 0-based lid of a 1-based id, or -1: a local id out of 1..nl
// (BoundsError), a global id absent from the gid table (KeyError)
template <bool GLOBAL, typename IT>
__device__ inline int64_t vec_lid(IT id, const uint64_t* __restrict__ sgid, const int64_t* __restrict__ slid,
                                  int64_t nl) {
  if (GLOBAL) return gid_lookup((int64_t)id, sgid, slid, nl);
  const int64_t l = (int64_t)id - 1;
  return (l < 0 || l >= nl) ? -1 : l;
}

// key[k] = the lid of id k, pay[k] = k; *bad = 1 when an id has no lid
template <bool GLOBAL, typename IT, typename K, typename P>
__global__ void k_vec_keys(int64_t n, const IT* __restrict__ I, const uint64_t* __restrict__ sgid,
                           const int64_t* __restrict__ slid, int64_t nl, K* __restrict__ key, P* __restrict__ pay,
                           int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = vec_lid<GLOBAL>(I[k], sgid, slid, nl);
    if (l < 0) *bad = 1;
    key[k] = l < 0 ? (K)0 : (K)l;
    pay[k] = (P)k;
  }
}

// to_lids!: the ids become 1-based lids (before the sort, key is in input order)
template <typename K>
__global__ void k_vec_lids_out(int64_t n, const K* __restrict__ key, int64_t* __restrict__ I) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
    I[k] = (int64_t)key[k] + 1;
}

// key sorted (stable), pay the input positions.  The thread at the first
// entry of a lid owns it: add: acc = v[lid]; acc = acc + V[..] over the lid's
// entries in input order; set: the last entry in input order.  Every key is
// below nl (k_vec_keys, checked by the caller before this pass).
template <typename T, typename K, typename P, bool SET>
__global__ void k_vec_scatter(int64_t n, const K* __restrict__ key, const P* __restrict__ pay,
                              const T* __restrict__ V, T* __restrict__ v) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const K l = key[k];
    if (k > 0 && key[k - 1] == l) continue;
    int64_t e = k + 1;
    if (SET) {
      while (e < n && key[e] == l) ++e;
      v[l] = V[pay[e - 1]];
    } else {
      T acc = v[l];
      acc = acc + V[pay[k]];
      for (; e < n && key[e] == l; ++e) acc = acc + V[pay[e]];
      v[l] = acc;
    }
  }
}

// out[k] = v[lid(id k)]; an id without a lid reads zero(T), and sets *bad
// unless absent_zero: an absent global id that may read as zero (LocalView,
// 2019-2026), or the 0 that mat_entry_ids gives an entry without a value
template <typename T, bool GLOBAL, typename IT>
__global__ void k_vec_gather(int64_t n, const IT* __restrict__ I, const uint64_t* __restrict__ sgid,
                             const int64_t* __restrict__ slid, int64_t nl, const T* __restrict__ v,
                             T* __restrict__ out, int absent_zero, int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = vec_lid<GLOBAL>(I[k], sgid, slid, nl);
    if (l < 0 && !absent_zero) *bad = 1;
    out[k] = l < 0 ? zero_of<T>() : v[l];
  }
}

namespace {

template <typename K, typename P>
void vec_keys(bool global, int index_bytes, int64_t n, const void* I, const uint64_t* sgid, const int64_t* slid,
              int64_t nl, K* key, P* pay, int* bad, hipStream_t st) {
  if (global)
    hipLaunchKernelGGL((k_vec_keys<true, int64_t, K, P>), grid1(n), dim3(256), 0, st, n, (const int64_t*)I, sgid,
                       slid, nl, key, pay, bad);
  else if (index_bytes == 8)
    hipLaunchKernelGGL((k_vec_keys<false, int64_t, K, P>), grid1(n), dim3(256), 0, st, n, (const int64_t*)I, sgid,
                       slid, nl, key, pay, bad);
  else
    hipLaunchKernelGGL((k_vec_keys<false, int32_t, K, P>), grid1(n), dim3(256), 0, st, n, (const int32_t*)I, sgid,
                       slid, nl, key, pay, bad);
}

template <typename T, typename K, typename P>
void vec_scatter_t(bool set, int64_t n, const K* key, const P* pay, const void* V, void* v, hipStream_t st) {
  if (set)
    hipLaunchKernelGGL((k_vec_scatter<T, K, P, true>), grid1(n), dim3(256), 0, st, n, key, pay, (const T*)V, (T*)v);
  else
    hipLaunchKernelGGL((k_vec_scatter<T, K, P, false>), grid1(n), dim3(256), 0, st, n, key, pay, (const T*)V, (T*)v);
}

// the scatter with keys of type K and payloads of type P (n >= 1)
template <typename K, typename P>
int vec_scatter_kp(int dtype, int64_t nl, void* v, bool global, int index_bytes, bool set, bool zero_first,
                   int64_t n, void* I, const void* V, const uint64_t* sgid, const int64_t* slid, hipStream_t st) {
  DevBuf<K> key;
  DevBuf<P> pay;
  DevBuf<int> bad;
  int hbad = 0;
  PA_HIP_OR(key.alloc(n), -1);
  PA_HIP_OR(pay.alloc(n), -1);
  PA_HIP_OR(bad.alloc(1), -1);
  PA_HIP_OR(hipMemsetAsync(bad, 0, sizeof(int), st), -1);
  vec_keys<K, P>(global, index_bytes, n, I, sgid, slid, nl, key.p, pay.p, bad.p, st);
  PA_HIP_OR(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);
  if (hbad) return 1;  // nothing written so far
  if (global) hipLaunchKernelGGL(k_vec_lids_out<K>, grid1(n), dim3(256), 0, st, n, key.p, (int64_t*)I);
  if (zero_first) PA_HIP_OR(hipMemsetAsync(v, 0, (size_t)nl * dtype_size(dtype), st), -1);
  PA_HIP_OR(sort_pairs(key, pay, n, bits_for((uint64_t)(nl - 1)), st), -1);
  switch (dtype) {
    case PA_F32: vec_scatter_t<float, K, P>(set, n, key, pay, V, v, st); break;
    case PA_F64: vec_scatter_t<double, K, P>(set, n, key, pay, V, v, st); break;
    case PA_C64: vec_scatter_t<c64, K, P>(set, n, key, pay, V, v, st); break;
    case PA_C128: vec_scatter_t<c128, K, P>(set, n, key, pay, V, v, st); break;
  }
  PA_HIP_OR(hipGetLastError(), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);  // key, pay and the caller's copies of I, V are freed on return
  return 0;
}

template <typename T>
void vec_gather_t(bool global, int index_bytes, int64_t n, const void* I, const uint64_t* sgid, const int64_t* slid,
                  int64_t nl, const void* v, void* out, int absent_zero, int* bad, hipStream_t st) {
  if (global)
    hipLaunchKernelGGL((k_vec_gather<T, true, int64_t>), grid1(n), dim3(256), 0, st, n, (const int64_t*)I, sgid,
                       slid, nl, (const T*)v, (T*)out, absent_zero, bad);
  else if (index_bytes == 8)
    hipLaunchKernelGGL((k_vec_gather<T, false, int64_t>), grid1(n), dim3(256), 0, st, n, (const int64_t*)I, sgid,
                       slid, nl, (const T*)v, (T*)out, absent_zero, bad);
  else
    hipLaunchKernelGGL((k_vec_gather<T, false, int32_t>), grid1(n), dim3(256), 0, st, n, (const int32_t*)I, sgid,
                       slid, nl, (const T*)v, (T*)out, absent_zero, bad);
}

}  // namespace

// One part's ordered scatter: v (nl values of dtype) takes the n pairs
// (I[k], V[k]) — I: 1-based lids (index_bytes 4 or 8) or, global, 1-based
// Int64 gids looked up in (sgid, slid) and overwritten by their 1-based lids;
// set: the last entry of a lid in input order is stored, else the entries are
// added to v[lid] in input order, from zero(T) everywhere when zero_first.
// I, V: device arrays.  wide: 64-bit sort keys and payloads (needed when nl
// or n exceeds 32 bits).  Returns 1 when an id has no lid (v and I are then
// unchanged), -1 on a HIP error.  The work is complete on return.
int vec_scatter(int dtype, int64_t nl, void* v, bool global, int index_bytes, bool set, bool zero_first, bool wide,
                int64_t n, void* I, const void* V, const uint64_t* sgid, const int64_t* slid, hipStream_t st) {
  if (n <= 0) {
    if (zero_first && nl > 0) PA_HIP_OR(hipMemsetAsync(v, 0, (size_t)nl * dtype_size(dtype), st), -1);
    return 0;
  }
  if (nl <= 0) return 1;  // no id has a lid
  if (wide) return vec_scatter_kp<uint64_t, int64_t>(dtype, nl, v, global, index_bytes, set, zero_first, n, I, V,
                                                     sgid, slid, st);
  return vec_scatter_kp<uint32_t, uint32_t>(dtype, nl, v, global, index_bytes, set, zero_first, n, I, V, sgid, slid,
                                            st);
}

// One part's gather: out[k] = v[lid of I[k]] (I, out: device arrays, n
// entries).  absent_zero: an id without a lid reads zero(T) (pa_vec_gather
// asks for it with global ids only); otherwise the call returns 1 (out is
// then unspecified).
// -1 on a HIP error.  The work is complete on return.
int vec_gather(int dtype, int64_t nl, const void* v, bool global, int index_bytes, bool absent_zero, int64_t n,
               const void* I, void* out, const uint64_t* sgid, const int64_t* slid, hipStream_t st) {
  if (n <= 0) return 0;
  DevBuf<int> bad;
  int hbad = 0;
  PA_HIP_OR(bad.alloc(1), -1);
  PA_HIP_OR(hipMemsetAsync(bad, 0, sizeof(int), st), -1);
  switch (dtype) {
    case PA_F32: vec_gather_t<float>(global, index_bytes, n, I, sgid, slid, nl, v, out, absent_zero, bad, st); break;
    case PA_F64: vec_gather_t<double>(global, index_bytes, n, I, sgid, slid, nl, v, out, absent_zero, bad, st); break;
    case PA_C64: vec_gather_t<c64>(global, index_bytes, n, I, sgid, slid, nl, v, out, absent_zero, bad, st); break;
    case PA_C128: vec_gather_t<c128>(global, index_bytes, n, I, sgid, slid, nl, v, out, absent_zero, bad, st); break;
  }
  PA_HIP_OR(hipGetLastError(), -1);
  PA_HIP_OR(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);
  return hbad ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Entry views of a PSparseMatrix (Interfaces.jl:2277-2298; pa_mat_scatter /
// pa_mat_gather): the lookup from (row lid, col lid) to the value index in
// main.val.  The entry table is derived from the layout the matrix already
// keeps — the slots' columns, the long rows' CSR and the ghost rows' (row,
// col) pairs — so the parent's colptr / rowval are not needed: one pass over
// the value indices emits key = row_lid * ncols_lids + col_lid for every
// index that holds a stored entry, the emitted pairs are compacted and
// sorted by key, and a lookup is a binary search.

// what k_entry_emit reads of a matrix
struct EntrySrc {
  int64_t slots, n_gnz, n_lnz, nrows, nslices, ncols, n_long;
  int H, R;
  const int64_t* off;         // main.off
  const int32_t* col;         // main.col
  const int32_t* kind;        // pa_mat::d_kind (null: every slice blocked)
  const int32_t* oid_to_lid;  // of the rows (null: the identity)
  const int32_t* grc;         // pa_mat::d_ghost_rc
  const int32_t* long_row;
  const int64_t* long_ptr;
  const int32_t* long_col;
  // pa_mat_findnz (both switches 0 for the entry table): column-major keys
  // col_lid * nrl + row_lid, and the stored ghost rows left out
  int64_t nrl;
  int colmajor, owned_only;
};

// value index t of main.val: flag[t] = 1 and key[t] = its entry's key when
// it holds a stored entry, flag[t] = 0 for padding.  A slot t of slice s is
// entry k of the slice's row w: t = off[s] + (k*64 + lane)*R + rr with
// w = lane*R + rr (mat_from_visit, k_fill_slots), or w = rr*64 + lane in a
// Float32 delta16 slice of 4 rows per lane (k_delta16 moved its rows).
__global__ void k_entry_emit(EntrySrc a, uint64_t* __restrict__ key, int64_t* __restrict__ flag) {
  const int64_t nv = a.slots + a.n_gnz + a.n_lnz;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nv; t += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = -1, c = -1;  // row lid, col lid
    if (t < a.slots) {
      int64_t lo = 0, hi = a.nslices;  // the last slice whose offset is <= t
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.off[mid] <= t) lo = mid; else hi = mid;
      }
      const int64_t u = t - a.off[lo];
      const int pos = (int)(u % a.H), lane = pos / a.R, rr = pos % a.R;
      const bool il = a.R == 4 && a.kind && a.kind[lo] == kBkDelta16;
      const int64_t oid = lo * a.H + (il ? rr * 64 + lane : lane * a.R + rr);
      c = a.col[t];
      if (oid < a.nrows && c >= 0) r = a.oid_to_lid ? a.oid_to_lid[oid] : oid;
    } else if (t < a.slots + a.n_gnz) {
      const int64_t g = t - a.slots;
      if (!a.owned_only) {
        r = a.grc[2 * g];
        c = a.grc[2 * g + 1];
      }
    } else {
      const int64_t q = t - a.slots - a.n_gnz;
      int64_t lo = 0, hi = a.n_long;  // the long row whose CSR range holds q
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.long_ptr[mid] <= q) lo = mid; else hi = mid;
      }
      const int64_t oid = a.long_row[lo];
      c = a.long_col[q];
      r = a.oid_to_lid ? a.oid_to_lid[oid] : oid;
    }
    const bool ok = r >= 0 && c >= 0;
    flag[t] = ok ? 1 : 0;
    key[t] = !ok ? 0
             : a.colmajor ? (uint64_t)c * (uint64_t)a.nrl + (uint64_t)r
                          : (uint64_t)r * (uint64_t)a.ncols + (uint64_t)c;
  }
}

// rank = exclusive scan of flag: the flagged value indices, in order
__global__ void k_entry_compact(int64_t nv, const uint64_t* __restrict__ key, const int64_t* __restrict__ flag,
                                const int64_t* __restrict__ rank, uint64_t* __restrict__ ekey,
                                int64_t* __restrict__ eidx) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nv; t += (int64_t)gridDim.x * blockDim.x)
    if (flag[t]) {
      ekey[rank[t]] = key[t];
      eidx[rank[t]] = t;
    }
}

// vidx[k] = 1 + the value index of entry (I[k], J[k]), or 0.  bad[0]: an id
// without a lid (absent_zero: an absent global id is none); bad[1]: a valid
// (i, j) the table does not hold.
template <bool GLOBAL, typename IT>
__global__ void k_entry_ids(int64_t n, const IT* __restrict__ I, const IT* __restrict__ J,
                            const uint64_t* __restrict__ rsgid, const int64_t* __restrict__ rslid, int64_t nrl,
                            const uint64_t* __restrict__ csgid, const int64_t* __restrict__ cslid, int64_t ncl,
                            const uint64_t* __restrict__ ekey, const int64_t* __restrict__ eidx, int64_t ne,
                            int absent_zero, int64_t* __restrict__ vidx, int* __restrict__ bad) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = vec_lid<GLOBAL>(I[k], rsgid, rslid, nrl);
    const int64_t j = vec_lid<GLOBAL>(J[k], csgid, cslid, ncl);
    int64_t v = 0;
    if (i < 0 || j < 0) {
      if (!(GLOBAL && absent_zero)) bad[0] = 1;
    } else {
      const uint64_t q = (uint64_t)i * (uint64_t)ncl + (uint64_t)j;
      int64_t lo = 0, hi = ne;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ekey[mid] < q) lo = mid + 1; else hi = mid;
      }
      if (lo < ne && ekey[lo] == q) v = eidx[lo] + 1;
      else bad[1] = 1;
    }
    vidx[k] = v;
  }
}

// the stored entries of A as (key, value index) pairs sorted by key, into
// ekey / eidx (*ne_out of them; none: both left empty).  colmajor: the key
// is col_lid * nrows_lids + row_lid, else row_lid * ncols_lids + col_lid;
// owned_only leaves the stored ghost rows out.  Emit over the value indices,
// scan, compact, sort.
static int entry_pairs(const pa_mat* A, const pa_index* rows, bool colmajor, bool owned_only, DevBuf<uint64_t>& ekey,
                       DevBuf<int64_t>& eidx, int64_t* ne_out, hipStream_t st) {
  const int64_t nv = A->main.slots + A->n_gnz + A->n_lnz;
  int64_t ne = 0;
  ekey.reset(), eidx.reset();
  *ne_out = 0;
  if (nv <= 0) return 0;
  DevBuf<uint64_t> key;
  DevBuf<int64_t> flag, rank;
  PA_HIP_OR(key.alloc(nv), -1);
  PA_HIP_OR(flag.alloc(nv), -1);
  PA_HIP_OR(rank.alloc(nv), -1);
  EntrySrc a;
  a.slots = A->main.slots, a.n_gnz = A->n_gnz, a.n_lnz = A->n_lnz;
  a.nrows = A->main.nrows, a.nslices = A->main.nslices, a.ncols = A->ncols_lids, a.n_long = A->n_long;
  a.H = A->H, a.R = A->R;
  a.off = A->main.off, a.col = A->main.col, a.kind = A->d_kind;
  a.oid_to_lid = rows->own_contig ? nullptr : rows->d_oid_to_lid.p;
  a.grc = A->d_ghost_rc;
  a.long_row = A->d_long_row, a.long_ptr = A->d_long_ptr, a.long_col = A->d_long_col;
  a.nrl = A->nrows_lids, a.colmajor = colmajor ? 1 : 0, a.owned_only = owned_only ? 1 : 0;
  hipLaunchKernelGGL(k_entry_emit, grid1(nv), dim3(256), 0, st, a, key.p, flag.p);
  PA_HIP_OR(hipGetLastError(), -1);
  PA_HIP_OR(scan_count(flag, rank, nv, st, &ne), -1);
  if (ne <= 0) return 0;
  PA_HIP_OR(ekey.alloc(ne), -1);
  PA_HIP_OR(eidx.alloc(ne), -1);
  hipLaunchKernelGGL(k_entry_compact, grid1(nv), dim3(256), 0, st, nv, key.p, flag.p, rank.p, ekey.p, eidx.p);
  PA_HIP_OR(hipGetLastError(), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);
  key.reset(), flag.reset(), rank.reset();  // before the sort takes its buffers
  // both lid counts guarded against 0 (a matrix without column lids stores
  // nothing and does not get here): the bits of the largest key of either order
  const uint64_t nrl = (uint64_t)(A->nrows_lids > 0 ? A->nrows_lids : 1);
  const uint64_t ncl = (uint64_t)(A->ncols_lids > 0 ? A->ncols_lids : 1);
  PA_HIP_OR(sort_pairs(ekey, eidx, ne, bits_for(nrl * ncl), st), -1);
  *ne_out = ne;
  return 0;
}

int mat_entry_table(pa_mat* A, const pa_index* rows, hipStream_t st) {
  if (entry_pairs(A, rows, false, false, A->d_ekey, A->d_eidx, &A->n_entries, st) != 0) return -1;
  A->has_entries = true;
  return 0;
}

int mat_entry_ids(const pa_mat* A, const pa_index* rows, const pa_index* cols, bool global, int index_bytes,
                  bool absent_zero, bool stored, int64_t n, const void* I, const void* J, int64_t* vidx,
                  hipStream_t st) {
  if (n <= 0) return 0;
  DevBuf<int> bad;
  int hbad[2] = {0, 0};
  PA_HIP_OR(bad.alloc(2), -1);
  PA_HIP_OR(hipMemsetAsync(bad, 0, 2 * sizeof(int), st), -1);
#define PA_ENTRY_IDS(G, IT)                                                                                          \
  hipLaunchKernelGGL((k_entry_ids<G, IT>), grid1(n), dim3(256), 0, st, n, (const IT*)I, (const IT*)J,                \
                     rows->d_sgid.p, rows->d_slid.p, rows->nlids, cols->d_sgid.p, cols->d_slid.p, cols->nlids,       \
                     A->d_ekey.p, A->d_eidx.p, A->n_entries, absent_zero ? 1 : 0, vidx, bad.p)
  if (global) {
    PA_ENTRY_IDS(true, int64_t);
  } else if (index_bytes == 8) {
    PA_ENTRY_IDS(false, int64_t);
  } else {
    PA_ENTRY_IDS(false, int32_t);
  }
#undef PA_ENTRY_IDS
  PA_HIP_OR(hipGetLastError(), -1);
  PA_HIP_OR(hipMemcpyAsync(hbad, bad, 2 * sizeof(int), hipMemcpyDeviceToHost, st), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);
  if (hbad[0]) return 1;
  return (stored && hbad[1]) ? 2 : 0;
}

// ---------------------------------------------------------------------------
// findnz / nziterator of a PSparseMatrix part (pa_mat_findnz; the filter of
// gather(A), Interfaces.jl:2671-2687): the stored entries back as (I, J, V)
// in the parent's storage order, the inverse of pa_mat_from_dcoo.
// entry_pairs, the routine that also builds the entry table, gives the
// (key, value index) pairs sorted by the key of the parent's order —
// col_lid * nrows_lids + row_lid for a CSC parent (SparseUtils.jl:106-150),
// row_lid * ncols_lids + col_lid for a CSR parent (254-300);
// k_findnz_write then splits each key into its ids and reads the entry's
// value from main.val, the one copy every layout is refreshed from.  The
// pairs land in the call's own buffers: the matrix's entry table is neither
// used nor built.

constexpr int kFindnzBlocks = 2048;  // grid of k_findnz_write (8 blocks per CU): kFindnzBlocks * 256 entries per grid pass

// entry k of the sorted pairs: I[k], J[k] = its ids (1-based lids, or gids
// through r2g / c2g), V[k] = val[eidx[k]].  Consecutive lanes write
// consecutive entries of I, J and V; the value reads are gathers.
template <typename T>
__global__ __launch_bounds__(256) void k_findnz_write(int64_t ne, const uint64_t* __restrict__ key,
                                                      const int64_t* __restrict__ eidx, uint64_t div, int colmajor,
                                                      const int64_t* __restrict__ r2g, const int64_t* __restrict__ c2g,
                                                      const T* __restrict__ val, int64_t* __restrict__ I,
                                                      int64_t* __restrict__ J, T* __restrict__ V) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < ne; k += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t q = key[k];
    const uint64_t hi = q / div, lo = q - hi * div;
    const int64_t r = (int64_t)(colmajor ? lo : hi), c = (int64_t)(colmajor ? hi : lo);
    const T v = val[eidx[k]];
    I[k] = r2g ? r2g[r] : r + 1;
    J[k] = c2g ? c2g[c] : c + 1;
    V[k] = v;
  }
}

template <typename T>
static void findnz_write_t(int64_t ne, const uint64_t* key, const int64_t* eidx, uint64_t div, int colmajor,
                           const int64_t* r2g, const int64_t* c2g, const void* val, CooList& out, hipStream_t st) {
  int64_t g = (ne + 255) / 256;
  if (g > kFindnzBlocks) g = kFindnzBlocks;
  hipLaunchKernelGGL(k_findnz_write<T>, dim3((unsigned)g), dim3(256), 0, st, ne, key, eidx, div, colmajor, r2g, c2g,
                     (const T*)val, out.I.p, out.J.p, (T*)out.V.p);
}

int mat_findnz(const pa_mat* A, const pa_index* rows, const pa_index* cols, bool owned_only, bool global,
               CooList& out, hipStream_t st) {
  out.I.reset(), out.J.reset(), out.V.reset();
  out.n = 0;
  const int colmajor = A->csr ? 0 : 1;
  DevBuf<uint64_t> ekey;
  DevBuf<int64_t> eidx;
  int64_t ne = 0;
  if (entry_pairs(A, rows, colmajor != 0, owned_only, ekey, eidx, &ne, st) != 0) return -1;
  if (ne <= 0) return 0;
  const uint64_t nrl = (uint64_t)(A->nrows_lids > 0 ? A->nrows_lids : 1);
  const uint64_t ncl = (uint64_t)(A->ncols_lids > 0 ? A->ncols_lids : 1);
  PA_HIP_OR(out.I.alloc(ne), -1);
  PA_HIP_OR(out.J.alloc(ne), -1);
  PA_HIP_OR(out.V.alloc(ne * dtype_size(A->dtype)), -1);
  const int64_t* r2g = global ? rows->d_lid_to_gid.p : nullptr;
  const int64_t* c2g = global ? cols->d_lid_to_gid.p : nullptr;
  const uint64_t div = colmajor ? nrl : ncl;
  switch (A->dtype) {
    case PA_F32: findnz_write_t<float>(ne, ekey, eidx, div, colmajor, r2g, c2g, A->main.val, out, st); break;
    case PA_F64: findnz_write_t<double>(ne, ekey, eidx, div, colmajor, r2g, c2g, A->main.val, out, st); break;
    case PA_C64: findnz_write_t<c64>(ne, ekey, eidx, div, colmajor, r2g, c2g, A->main.val, out, st); break;
    case PA_C128: findnz_write_t<c128>(ne, ekey, eidx, div, colmajor, r2g, c2g, A->main.val, out, st); break;
  }
  PA_HIP_OR(hipGetLastError(), -1);
  PA_HIP_OR(hipStreamSynchronize(st), -1);
  out.n = ne;
  return 0;
}

}  // namespace pa

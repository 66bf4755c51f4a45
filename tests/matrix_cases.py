"""Matrix generators shared by the GPU test modules (plain helpers, no
fixtures): each returns host triplets or a host CSR; the tests build the
device matrices from them."""
import numpy as np

SEED = 20250114


def rand(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def long_row_coo(rng, part, p, dtype, long_lens):
    """owned rows with ~9 entries, a few rows with long_lens entries (over all
    local columns, ghosts included), in random order with duplicates."""
    s = part.partition.local(p)
    own = s.oid_to_lid
    I, J = [], []
    longs = rng.choice(own, size=min(len(long_lens), len(own)), replace=False)
    for li in own:
        k = 9
        if li in longs:
            k = long_lens[list(longs).index(li)]
        I += [li] * k
        J += list(rng.integers(1, s.num_lids + 1, size=k))
    I, J = np.array(I), np.array(J)
    o = rng.permutation(len(I))
    V = rng.uniform(-1, 1, len(I))
    if np.dtype(dtype).kind == "c":
        V = V + 1j * rng.uniform(-1, 1, len(I))
    return I[o], J[o], V[o].astype(dtype), sorted(int(v) for v in longs)


def unsorted_csr(n, D, Bi, order, dtype):
    """rowptr, colval (Bi-based), nzval of the band matrix with every row
    stored diagonal first and the others ascending, or descending; the
    triplets in that order too."""
    rows, cols = [], []
    for i in range(n):
        js = [i + d for d in sorted(D) if 0 <= i + d < n]
        js = ([i] + [j for j in js if j != i]) if order == "diag_first" else js[::-1]
        rows += [i] * len(js)
        cols += js
    I, J = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=n))]).astype(np.int64) + Bi
    rng = np.random.default_rng([SEED, 13, n, len(D)])
    V = rand(rng, len(I), dtype)
    return rowptr, J + Bi, V, I + 1, J + 1, rand(rng, n, dtype)


def with_ghost_coo(rows, parts, ngids, periodic, rng):
    """global-id COO of a 7-point operator with random coefficients over each
    part's owned rows (neighbours wrap around periodic dimensions)."""
    D = len(ngids)
    per = periodic or (False,) * D
    I, J, V = {}, {}, {}
    for p in parts.part_ids:
        s = rows.partition.local(p)
        own = s.lid_to_gid[s.oid_to_lid - 1]
        ci = [(own - 1) // int(np.prod(ngids[:d])) % ngids[d] for d in range(D)]
        ii, jj = [own], [own]
        for d in range(D):
            for step in (-1, 1):
                c = ci[d] + step
                ok = np.ones(len(own), bool) if per[d] else (c >= 0) & (c < ngids[d])
                c = c % ngids[d]
                nb = own + (c - ci[d]) * int(np.prod(ngids[:d]))
                ii.append(own[ok])
                jj.append(nb[ok])
        I[p] = np.concatenate(ii)
        J[p] = np.concatenate(jj)
        V[p] = rng.uniform(-1, 1, len(I[p]))
    return I, J, V


def tridiag(n, part_rows):
    """global-id COO of the owned rows of a 1-D Laplacian-like matrix."""
    I, J, V = [], [], []
    for g in part_rows:
        for d, v in ((-1, -1.0), (0, 4.0), (1, -1.5)):
            if 1 <= g + d <= n:
                I.append(g)
                J.append(g + d)
                V.append(v + 0.01 * g)
    return np.array(I, np.int64), np.array(J, np.int64), np.array(V)

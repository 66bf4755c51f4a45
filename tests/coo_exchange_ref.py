"""exchange!(I, J, V, rows) restated from the reference (Interfaces.jl:
2494-2592) on the oracle's pieces, as oracle/pa_oracle.py assemble_coo_
restates 2406-2492, plus the random COO problems and the per-triplet
classification the exchange tests share.  Not a test module."""
import numpy as np


def exchange_coo_(O, I, J, V, rows):
    """async_exchange!(I, J, V, rows) + wait.  I, J: PData of lists of global
    ids (changed in place), V: PData of numpy arrays (ghost rows' unsent
    values are zeroed in place).  Returns I, J and the new V."""
    O.to_lids_pr_(I, rows)                                                   # 2508
    parts = O.get_part_ids(rows.partition.shape if len(rows.partition.shape) > 1 else O.num_parts(rows.partition))
    ex = rows.exchanger

    vdt = np.asarray(V.parts[0] if V.parts else []).dtype
    vdt = vdt if vdt.kind in "fc" else np.dtype(np.float64)

    def setup_snd(part, psnd, lsnd, s, i, j, v):                             # 2511-2556
        unset = 0
        lid_to_i = [unset] * s.num_lids
        for ii in range(1, len(lsnd) + 1):                                   # 2515-2520
            for p in range(lsnd.ptrs[ii - 1], lsnd.ptrs[ii]):
                lid = lsnd.data[p - 1]
                lid_to_i[lid - 1] = ii                                       # overwritten: the last segment stays
        for k in range(len(i)):                                              # 2524-2532
            li = i[k]
            ii = lid_to_i[li - 1]
            if ii != unset:
                pass                                                         # ptrs[i+1] += 1
            elif s.lid_to_part[li - 1] != part:
                v[k] = vdt.type(0)                                           # zero(Tv): not v*0
        segs = [[[], [], []] for _ in psnd]
        for k in range(len(i)):                                              # 2537-2550
            li = i[k]
            ii = lid_to_i[li - 1]
            if ii != unset:
                seg = segs[ii - 1]
                seg[0].append(s.lid_to_gid[li - 1])
                seg[1].append(j[k])
                seg[2].append(v[k])
        return segs
    segs = O.map_parts(setup_snd, parts, ex.parts_snd, ex.lids_snd, rows.partition, I, J, V)
    got = []
    for t in range(3):                                                       # 2561-2563
        data = O.map_parts(lambda sg: O.table_from([x[t] for x in sg], dtype=vdt if t == 2 else np.int64), segs)
        got.append(O.exchange_tables(data, ex.parts_rcv, ex.parts_snd))

    def setup_rcv(s, i, j, v, gi, gj, gv):                                   # 2565-2587
        O.to_gids_(i, s)
        i.extend(int(x) for x in gi.data)
        j.extend(int(x) for x in gj.data)
        return np.concatenate([np.asarray(v, dtype=vdt), gv.data.astype(vdt)])
    V2 = O.map_parts(setup_rcv, rows.partition, I, J, V, *got)
    return I, J, V2


def rand_values(rng, n, dtype):
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def problem(pamd, O, be, nparts, ngids, m, dtype, seed, with_ghost=False, remote_frac=0.25):
    """rows (product and oracle) and a random COO per part, drawn as
    test_gpu_coo_assemble._problem draws it: 75 % of the rows among the
    part's owned gids, 25 % any gid, then add_gids!(rows, I).  `be`: any
    backend of the product (the sequential one for host-only use)."""
    parts = be.get_part_ids(nparts)
    oparts = O.get_part_ids(nparts)
    if isinstance(ngids, tuple):
        rows = pamd.prange_cartesian(parts, ngids, with_ghost=with_ghost)
        orows = O.prange_cartesian(oparts, ngids, with_ghost=with_ghost)
        ntot = int(np.prod(ngids))
    else:
        rows, orows = pamd.prange_linear(parts, ngids), O.prange_linear(oparts, ngids)
        ntot = ngids
    rng = np.random.default_rng(seed)
    I, J, V = {}, {}, {}
    for p in parts.part_ids:
        s = rows.partition.local(p)
        own = s.lid_to_gid[s.oid_to_lid - 1]
        k = m
        nrem = int(k * remote_frac)
        i = np.concatenate([rng.choice(own, k - nrem), rng.integers(1, ntot + 1, nrem)])
        rng.shuffle(i)
        I[p] = i.astype(np.int64)
        J[p] = rng.integers(1, ntot + 1, k).astype(np.int64)
        V[p] = rand_values(rng, k, dtype)
    mk = lambda d: pamd.PData(parts.backend, parts.part_ids, [d[p].copy() for p in parts.part_ids], parts.shape)
    pamd.add_gids_(rows, mk(I))
    O.add_gids_(orows, O.PData([list(map(int, I[p])) for p in parts.part_ids], oparts.shape))
    return parts, oparts, rows, orows, I, J, V, mk


def classify(orows, part_ids, I):
    """per part, per triplet: (kind, nlisted) with kind 1 = sent (its lid is
    in a send segment), 2 = an unsent ghost row (value zeroed), 0 = neither;
    nlisted = the number of send segments that list the lid"""
    out = {}
    for p in part_ids:
        s = orows.partition[p]
        lsnd = orows.exchanger.lids_snd[p]
        listed = np.zeros(s.num_lids, dtype=np.int64)
        for seg in lsnd.tolist():
            for lid in set(int(x) for x in seg):
                listed[lid - 1] += 1
        lids = np.array([s.gid_to_lid[int(g)] for g in I[p]], dtype=np.int64)
        ghost = np.array(s.lid_to_part, dtype=np.int64) != s.part
        n = listed[lids - 1] if len(lids) else np.zeros(0, np.int64)
        kind = np.where(n > 0, 1, np.where(ghost[lids - 1], 2, 0)) if len(lids) else np.zeros(0, np.int64)
        out[p] = (kind, n)
    return out


def oracle_lists(O, part_ids, oparts, I, J, V):
    return (O.PData([list(map(int, I[p])) for p in part_ids], oparts.shape),
            O.PData([list(map(int, J[p])) for p in part_ids], oparts.shape),
            O.PData([V[p].copy() for p in part_ids], oparts.shape))

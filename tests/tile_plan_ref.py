"""Plain-Python restatement of the tile planner of p2m_graph_create (csrc/capi.hip: merged-row pattern, fake-vertex rule,
locality_order, build_tile_plan for the three plans of a level) and generators of graphs that drive the plans to the caps
of csrc/p2m_common.h (TILE_RMAX rows, TILE_UCAP union rows, TILE_ECAP entries per tile).  No GPU, no library: the GPU tests
compare the library's planner with this one, and take the rows of every tile from it.

A plan is None (the library reports 0 tiles: the row kernel stays in charge) or a list with one tuple per tile:
(first compact row, rows, union size, entries, padded entries = sum of the row lengths rounded up to 4)."""
import numpy as np
import scipy.sparse as sp

RMAX, UCAP, ECAP = 32, 120, 896            # TILE_RMAX, TILE_UCAP, TILE_ECAP
MIN_REAL, MIN_PAIR = 256, 128              # plans at all: n_fake > 0 and n_real >= 256; paired plan: >= 128 paired real rows


def laplacian(A, V):
    """(I - D^-1/2 A D^-1/2) / 3 - I with isolated (diagonal-only) vertices, built as tests/test_gpu_ops.py:_band_graph does."""
    A = sp.csr_matrix(A, shape=(V, V))
    A.data[:] = 1.0
    d = np.asarray(A.sum(axis=0)).ravel() + np.spacing(np.float64(0))
    Dm = sp.diags(1 / np.sqrt(d))
    return ((sp.identity(V) - Dm @ A @ Dm) / 3.0 - sp.identity(V)).tocsr()


def permuted(L, seed):
    """Random renumbering of ALL vertices: the isolated fake vertices end up anywhere, as in a coarsening tree."""
    V = L.shape[0]
    perm = np.random.default_rng(seed).permutation(V)
    return L.tocsr()[perm][:, perm].tocsr()


def _sym(rows, cols, V):
    r = np.concatenate([rows, cols])
    c = np.concatenate([cols, rows])
    return sp.coo_matrix((np.ones(r.size), (r, c)), shape=(V, V)).tocsr()


def _csr(L):
    """The CSR that ops.DeviceGraph hands to the library (duplicates summed, sorted columns, explicit zeros kept)."""
    L = sp.csr_matrix(L, dtype=np.float64)
    L.sum_duplicates()
    L.sort_indices()
    return L


def merged_pattern(L):
    """Row pointer and sorted columns of the merged rows: pattern of L, of L L and the diagonal."""
    V = L.shape[0]
    P = sp.csr_matrix((np.ones(L.nnz), L.indices, L.indptr), shape=L.shape)
    M = (P @ P + P + sp.identity(V)).tocsr()
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int64)


def fake_mask(L, rp, mc):
    """Fake (isolated) vertices: merged rows with the diagonal as their only entry that share the most common (a, b) pair,
    a = fp32(L_ii), b = fp32(2 L_ii^2 - 1) (ties: the smallest pair, the first key of the library's ordered map)."""
    V = L.shape[0]
    lens = np.diff(rp)
    lone = (lens == 1) & (mc[rp[:-1].clip(max=len(mc) - 1)] == np.arange(V))
    fake = np.zeros(V, bool)
    if not lone.any():
        return fake
    ids = np.where(lone)[0]
    # a lone merged row has a lone row of L (its diagonal) or an empty one
    val = np.array([L.data[L.indptr[i]].astype(np.float32) if L.indptr[i + 1] > L.indptr[i] else np.float32(0) for i in ids],
                   dtype=np.float32).astype(np.float64)
    has = np.array([L.indptr[i + 1] > L.indptr[i] for i in ids])
    a = val.astype(np.float32)
    b = (np.where(has, 2.0 * val * val, 0.0) - 1.0).astype(np.float32)
    count = {}
    for x, y in zip(a.tolist(), b.tolist()):
        count[(x, y)] = count.get((x, y), 0) + 1
    best = max(count.values())
    fa, fb = min(k for k, c in count.items() if c == best)
    fake[ids[(a == np.float32(fa)) & (b == np.float32(fb))]] = True
    return fake


def locality_order(real_ids, V, row_ptr, col, rp, mc):
    """capi.hip locality_order: greedy patches; a patch starts at the boundary vertex with the most assigned neighbours and
    keeps adding the frontier vertex whose merged row adds the fewest new union columns, until 32 rows or a cap."""
    n = len(real_ids)
    isreal = np.zeros(V, bool)
    isreal[real_ids] = True
    assigned = np.zeros(V, bool)
    infront = np.zeros(V, bool)
    inbound = np.zeros(V, bool)
    cnt = np.zeros(V, np.int64)
    stamp = -np.ones(V, np.int64)
    rows_mc = [mc[rp[v]:rp[v + 1]] for v in range(V)]
    rows_l = [col[row_ptr[v]:row_ptr[v + 1]] for v in range(V)]
    order, boundary = [], []
    done = nxt = patch = 0
    while done < n:
        seed, best = -1, -1
        keep = []
        for v in boundary:
            if assigned[v]:
                continue
            keep.append(v)
            if cnt[v] > best or (cnt[v] == best and v < seed):
                best, seed = cnt[v], v
        boundary = keep
        if seed < 0:
            while assigned[real_ids[nxt]]:
                nxt += 1
            seed = int(real_ids[nxt])
        patch += 1
        front = []
        rows = usize = entries = 0
        cur = seed
        while True:
            cols = rows_mc[cur]
            new = cols[stamp[cols] != patch]
            stamp[new] = patch
            usize += len(new)
            entries += len(cols)
            assigned[cur] = True
            order.append(cur)
            rows += 1
            done += 1
            for w in rows_l[cur].tolist():
                cnt[w] += 1
                if isreal[w] and not assigned[w] and not infront[w]:
                    infront[w] = True
                    front.append(w)
            if rows >= RMAX:
                break
            pick, pick_new = -1, 1 << 30
            for w in front:
                if assigned[w]:
                    continue
                nw = int(np.count_nonzero(stamp[rows_mc[w]] != patch))
                if nw < pick_new or (nw == pick_new and w < pick):
                    pick_new, pick = nw, w
            if pick < 0 or usize + pick_new > UCAP or entries + len(rows_mc[pick]) > ECAP:
                break
            cur = pick
        for w in front:
            infront[w] = False
            if not assigned[w] and not inbound[w]:
                inbound[w] = True
                boundary.append(w)
    return np.asarray(order, dtype=np.int64)


def build_tile_plan(rows_src):
    """capi.hip build_tile_plan on rows given as arrays of source ids (repeats = separate entries, one union column)."""
    tiles = []
    i, n = 0, len(rows_src)
    while i < n:
        uni = set()
        rows = entries = padded = 0
        while i + rows < n and rows < RMAX:
            r = rows_src[i + rows]
            nu = uni | set(r.tolist())
            if rows > 0 and (len(nu) > UCAP or entries + len(r) > ECAP):
                break
            uni = nu
            entries += len(r)
            padded += (len(r) + 3) & ~3
            rows += 1
        if len(uni) > UCAP or entries > ECAP:
            return None                                  # a single row too large: no plan
        tiles.append((i, rows, len(uni), entries, padded))
        i += rows
    return tiles or None


class Plans:
    """What the library should have planned for one level.  plan[p]: None or the tiles; row_len[p]: entries of every compact
    row of plan p; real_order: the real vertices in compact row order; pair_order: the coarse vertices of the paired plan."""

    def __init__(self, L, tree_order=False):
        L = _csr(L)
        V = L.shape[0]
        self.V = V
        rp, mc = merged_pattern(L)
        self.max_row = int(np.diff(rp).max())
        fake = fake_mask(L, rp, mc)
        self.fake = fake
        real_ids = np.where(~fake)[0]
        self.n_real, self.n_fake = int(real_ids.size), int(fake.sum())
        self.plan = [None, None, None]
        self.row_len = [None, None, None]
        self.real_order = real_ids
        self.pair_order = np.zeros(0, np.int64)
        if not (self.n_fake > 0 and self.n_real >= MIN_REAL):
            return
        if not tree_order:
            self.real_order = locality_order(real_ids, V, L.indptr, L.indices, rp, mc)
        for sh in (0, 1):
            if sh == 1 and (V & 1):
                break
            rows = [mc[rp[v]:rp[v + 1]] >> sh for v in self.real_order]
            self.plan[sh] = build_tile_plan(rows)
            self.row_len[sh] = np.array([len(r) for r in rows])
        if V & 1:
            return
        rows, pair = [], []
        for c in range(V // 2):
            u, w = 2 * c, 2 * c + 1
            if fake[u] and fake[w]:
                continue
            pair.append(c)
            rows.append(np.union1d(mc[rp[u]:rp[u + 1]], mc[rp[w]:rp[w + 1]]))
        if len(pair) >= MIN_PAIR:
            self.plan[2] = build_tile_plan(rows)
            self.row_len[2] = np.array([len(r) for r in rows])
            if self.plan[2] is not None:
                self.pair_order = np.asarray(pair, dtype=np.int64)

    @property
    def n_pair_real(self):
        return int(self.pair_order.size)

    @property
    def plan_tiles(self):
        return tuple(0 if p is None else len(p) for p in self.plan)

    def summary(self, p):
        """tiles / max rows / max union / max entries / max padded / one-row tiles of plan p (None: absent)."""
        if self.plan[p] is None:
            return None
        a = np.array(self.plan[p])
        return {"tiles": len(a), "rows_min": int(a[:, 1].min()), "rows_max": int(a[:, 1].max()),
                "union_max": int(a[:, 2].max()), "entries_max": int(a[:, 3].max()), "padded_max": int(a[:, 4].max()),
                "one_row": int((a[:, 1] == 1).sum()), "row_len_max": int(self.row_len[p].max())}

    def describe(self):
        return "; ".join(f"plan {p}: " + ("none" if self.plan[p] is None else
                                           "{tiles} tiles, rows {rows_min}-{rows_max}, union <= {union_max}, entries <= "
                                           "{entries_max}, padded <= {padded_max}, {one_row} one-row, longest row "
                                           "{row_len_max}".format(**self.summary(p))) for p in range(3))


# ---- graph families -----------------------------------------------------------------------------------------------------

def band(V, seed, fake_frac=0.4, nreal=None):
    """tests/test_gpu_ops.py:_band_graph (ring + chords 5 and 17 over the real vertices, all vertices renumbered).
    nreal: the number of real vertices, exactly (instead of the share 1 - fake_frac of V); the other V - nreal are isolated.
    The chords stay distinct from 35 real vertices up."""
    if nreal is None:
        nreal = max(8, int(V * (1 - fake_frac)))
    assert 8 <= nreal <= V
    i = np.arange(nreal)
    A = _sym(np.concatenate([i, i, i]), np.concatenate([(i + 1) % nreal, (i + 5) % nreal, (i + 17) % nreal]), V)
    return permuted(laplacian(A, V), seed)


def clique_size(n):
    """(cliques, V) of the cliques(n) family: at least 10 cliques and about 600 real vertices, 40 % isolated vertices."""
    k = max(10, 600 // n)
    return k, ((n * k * 5 // 3) + 31) // 32 * 32


def cliques(n, perm_seed=None):
    """k disjoint n-cliques on the first n k vertices: every merged row is its clique (n entries, union n)."""
    k, V = clique_size(n)
    rows, cols = [], []
    for q in range(k):
        ids = np.arange(q * n, (q + 1) * n)
        a, b = np.meshgrid(ids, ids)
        m = a < b
        rows.append(a[m])
        cols.append(b[m])
    L = laplacian(_sym(np.concatenate(rows), np.concatenate(cols), V), V)
    return L if perm_seed is None else permuted(L, perm_seed)


def hub(target, perm_seed=None, V=1472, nreal=900):
    """Band graph on nreal - 1 vertices + one hub (vertex nreal - 1) tied to 17 spokes 50 apart: the hub's merged row is
    itself, the spokes and their 6 band neighbours each = 120 columns.  target = 121: one pendant vertex (nreal) on spoke 0
    pushes the hub's row one past the cap."""
    assert target in (120, 121)
    n = nreal - 1
    i = np.arange(n)
    A = _sym(np.concatenate([i, i, i]), np.concatenate([(i + 1) % n, (i + 5) % n, (i + 17) % n]), V)
    A = A + _sym(np.full(17, n), np.arange(17) * 50, V)
    if target == 121:
        A = A + _sym(np.array([nreal]), np.array([0]), V)
    L = laplacian(A, V)
    return L if perm_seed is None else permuted(L, perm_seed)


def mixed(perm_seed=None, nreal=800, V=1472, seed=1):
    """Preferential attachment (3 ties per new vertex, weight degree^1.5); a tie is rejected if it pushes any 2-ring past the
    union cap.  Degrees 1 ... ~48, merged rows up to the cap, tiles whose rows differ widely in length.  The 2-rings are kept
    incrementally (a new tie u - v only grows the rings of u, v and their neighbours)."""
    rng = np.random.default_rng(seed)
    adj = [set() for _ in range(nreal)]
    ring = [{v} for v in range(nreal)]                   # v, its neighbours and theirs
    deg = np.ones(nreal)
    for v in range(1, nreal):
        for _ in range(3):
            p = deg[:v] ** 1.5
            u = int(rng.choice(v, p=p / p.sum()))
            if u in adj[v]:
                continue
            ok = len(ring[u] | adj[v] | {v}) <= UCAP and len(ring[v] | adj[u] | {u}) <= UCAP
            ok = ok and all(len(ring[x]) + (v not in ring[x]) <= UCAP for x in adj[u])
            ok = ok and all(len(ring[x]) + (u not in ring[x]) <= UCAP for x in adj[v])
            if not ok:
                continue
            ring[u] |= adj[v] | {v}
            ring[v] |= adj[u] | {u}
            for x in adj[u]:
                ring[x].add(v)
            for x in adj[v]:
                ring[x].add(u)
            adj[v].add(u)
            adj[u].add(v)
            deg[u] += 1
            deg[v] += 1
    r = np.array([v for v in range(nreal) for u in adj[v] if u > v])
    c = np.array([u for v in range(nreal) for u in adj[v] if u > v])
    L = laplacian(_sym(r, c, V), V)
    return L if perm_seed is None else permuted(L, perm_seed)


# name -> builder; the seeds of the renumberings are part of the cases (tests/test_tile_plan_cpu.py pins what they reach)
FAMILIES = {
    "cliques56": lambda: cliques(56), "cliques56p": lambda: cliques(56, 5),
    "cliques28": lambda: cliques(28), "cliques29": lambda: cliques(29),
    "cliques120": lambda: cliques(120), "cliques120p": lambda: cliques(120, 5),
    "cliques121": lambda: cliques(121),
    "hub120": lambda: hub(120), "hub120p": lambda: hub(120, 3),
    "hub121": lambda: hub(121), "hub121p": lambda: hub(121, 3),
    "mixed": lambda: mixed(), "mixedp": lambda: mixed(9),
}

_cache = {}


def family(name, tree_order=False):
    """(L, Plans) of a named family, built once per process."""
    key = (name, tree_order)
    if key not in _cache:
        L = _cache[(name, None)] if (name, None) in _cache else FAMILIES[name]()
        _cache[(name, None)] = L
        _cache[key] = (L, Plans(L, tree_order))
    return _cache[key]


def dense(L):
    return np.asarray(sp.csr_matrix(L).toarray(), dtype=np.float64)


if __name__ == "__main__":
    import sys
    import time
    for name in sys.argv[1:] or list(FAMILIES):
        t = time.time()
        L, p = family(name)
        print(f"{name}: V {p.V} n_real {p.n_real} n_fake {p.n_fake} pair {p.n_pair_real} max merged row {p.max_row} "
              f"({time.time() - t:.1f} s)\n   " + p.describe().replace("; ", "\n   "))

"""The definition of the UMI collapse (include/telescope_em.h, tsem_umi_dedup) on the host, for the tests.

`dedup_plain` IS the definition: dicts, sets and a union-find over rows — the truth every other form is compared with.
`dedup_vectorised` states it again with numpy / scipy (a bipartite row - (class, column) graph handed to
scipy.sparse.csgraph.connected_components): what a host implementation at scale would look like, and what the timing tool runs.

Both take the CSR arrays of the raw score codes and the two per-row maps and return (rep int32 [N], stats int64 [4]):
stats = rows in classes, classes, components among the rows in classes, rows dropped.
"""
import numpy as np


def dedup_plain(indptr, indices, data, cell_of_row, umi_of_row):
    n = len(indptr) - 1
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    classes = {}
    for i in range(n):
        c, u = int(cell_of_row[i]), int(umi_of_row[i])
        if c >= 0 and u >= 0:
            classes.setdefault((c, u), []).append(i)
    for rows in classes.values():
        first_with = {}                                      # column -> a row of the class that stores it
        for i in rows:
            for col in set(int(j) for j in indices[indptr[i]:indptr[i + 1]]):
                if col in first_with:
                    a, b = find(first_with[col]), find(i)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
                else:
                    first_with[col] = i
    members = {}
    for i in range(n):
        members.setdefault(find(i), []).append(i)
    rep = np.empty(n, np.int32)
    for rows in members.values():
        best = min(rows, key=lambda r: (-max([int(v) for v in data[indptr[r]:indptr[r + 1]]] + [-1]), r))
        for r in rows:
            rep[r] = best
    in_class = set(i for rows in classes.values() for i in rows)
    stats = np.array([len(in_class), len(classes), sum(1 for root in members if root in in_class),
                      n - int(np.sum(rep == np.arange(n)))], np.int64)
    return rep, stats


def dedup_vectorised(indptr, indices, data, cell_of_row, umi_of_row, n_cols=None):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    data = np.asarray(data, np.int64)
    cell, umi = np.asarray(cell_of_row, np.int64), np.asarray(umi_of_row, np.int64)
    n = len(indptr) - 1
    k = int(n_cols) if n_cols is not None else (int(indices.max()) + 1 if indices.size else 1)
    in_class = (cell >= 0) & (umi >= 0)
    n_class_rows = int(in_class.sum())
    cls = np.full(n, -1, np.int64)
    n_classes = 0
    if n_class_rows:
        n_umis = int(umi.max()) + 1
        _, inv = np.unique(cell[in_class] * n_umis + umi[in_class], return_inverse=True)
        cls[in_class] = inv
        n_classes = int(inv.max()) + 1
    lens = np.diff(indptr)
    row_of_entry = np.repeat(np.arange(n), lens)
    sel = cls[row_of_entry] >= 0
    er = row_of_entry[sel]
    _, node = np.unique(cls[er] * k + indices[sel], return_inverse=True)
    n_nodes = int(node.max()) + 1 if node.size else 0
    g = sp.coo_matrix((np.ones(er.size, np.int8), (er, n + node)), shape=(n + n_nodes, n + n_nodes))
    _, comp = connected_components(g, directed=False)
    comp = comp[:n]
    maxcode = np.full(n, -1, np.int64)
    has = lens > 0
    if has.any():
        maxcode[has] = np.maximum.reduceat(data, indptr[:-1][has])
    order = np.lexsort((np.arange(n), -maxcode, comp))       # by component, then the largest code first, then the row
    first = np.ones(n, bool)
    first[1:] = comp[order][1:] != comp[order][:-1]
    rep_of_comp = np.zeros(int(comp.max()) + 1 if n else 0, np.int64)
    rep_of_comp[comp[order][first]] = order[first]
    rep = rep_of_comp[comp].astype(np.int32) if n else np.zeros(0, np.int32)
    stats = np.array([n_class_rows, n_classes, len(np.unique(comp[in_class])), n - int(np.sum(rep == np.arange(n)))], np.int64)
    return rep, stats


def random_case(seed, n=3000, k=60, max_len=6, n_cells=12, n_umis=40):
    """The random cases of the GPU tests: row lengths uniform in 1..max_len, cells uniform in -1..n_cells - 1, UMIs uniform in
    -1..n_umis - 1, distinct column ids in no order."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, max_len + 1, n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([rng.permutation(k)[:ln] for ln in lens]).astype(np.int32)
    data = rng.integers(1, 300, int(indptr[-1])).astype(np.uint16)
    cell = rng.integers(-1, n_cells, n).astype(np.int32)
    umi = rng.integers(-1, n_umis, n).astype(np.int32)
    return indptr, indices, data, cell, umi, k


def ground(indptr, indices, data, cell, umi):
    """(rows dropped, components with >= 3 rows, classes that split into >= 2 components) by the plain reference."""
    rep, stats = dedup_plain(indptr, indices, data, cell, umi)
    # components: rows that share (class, rep)
    in_class = (np.asarray(cell) >= 0) & (np.asarray(umi) >= 0)
    sizes = np.bincount(rep[in_class], minlength=len(rep))
    per_class = {}
    for i in np.flatnonzero(in_class):
        per_class.setdefault((int(cell[i]), int(umi[i])), set()).add(int(rep[i]))
    return int(stats[3]), int(np.sum(sizes >= 3)), sum(1 for s in per_class.values() if len(s) >= 2)

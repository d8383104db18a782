"""numpy restatement of `general.separate_instances` (unscene3d_amd/trainer/separate.py), written from its five rules,
not from the device code:

  1  U = sorted unique ids of seg, S = len(U), idx(r) in [0, S)
  2  a — b iff BOTH (a, b) and (b, a) are listed; self pairs and pairs naming an id outside U are ignored
  3  segment s belongs to instance j iff ANY point of s has masks[:, j] set
  4  the parts of j are the connected components (union-find) of its segments, ordered by smallest segment index
  5  one column per (instance, part) in that order: all points whose segment is in the part
"""
import numpy as np


def mutual_adjacency(conn, unique_segments):
    """-> list of S sets of segment INDICES (rule 2)."""
    index = {int(s): i for i, s in enumerate(unique_segments)}
    listed = set()
    for a, b in np.asarray(conn, np.int64).reshape(-1, 2):
        ia, ib = index.get(int(a)), index.get(int(b))
        if ia is not None and ib is not None and ia != ib:
            listed.add((ia, ib))
    adj = [set() for _ in unique_segments]
    for ia, ib in listed:
        if (ib, ia) in listed:
            adj[ia].add(ib)
    return adj


def adjacency_csr(adj):
    """list of sets -> (off int64[S+1], nbr int32[E]) with ascending neighbours: the layout of `segment_adjacency`."""
    off = np.zeros(len(adj) + 1, np.int64)
    off[1:] = np.cumsum([len(a) for a in adj])
    nbr = np.array([t for a in adj for t in sorted(a)], np.int32).reshape(-1)
    return off, nbr


def components(mask, adj):
    """Union-find.  mask bool[S] -> int64[S]: -1 outside the mask, else the smallest index of the part."""
    mask = np.asarray(mask, bool)
    parent = np.arange(len(mask))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for s in np.nonzero(mask)[0]:
        for t in adj[s]:
            if mask[t]:
                a, b = find(s), find(t)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(s) if mask[s] else -1 for s in range(len(mask))], np.int64)


def segment_masks(masks, idx, S):
    """Rule 3: bool[N, K] -> bool[K, S]."""
    masks = np.asarray(masks) != 0
    out = np.zeros((masks.shape[1], S), bool)
    for j in range(masks.shape[1]):
        out[j, np.unique(idx[masks[:, j]])] = True
    return out


def pack_rows(rows):
    """bool[K, S] -> uint64[K, ceil(S/64)], segment s = bit s % 64 of word s / 64."""
    rows = np.asarray(rows, bool)
    K, S = rows.shape
    W = (S + 63) // 64
    padded = np.zeros((K, W * 64), np.uint8)
    padded[:, :S] = rows
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(K, W)


def separate_ref(masks, seg, conn):
    """-> (columns bool[N, R], src int64[R], parts: per column the sorted segment INDICES, uniq int64[S])."""
    seg = np.asarray(seg, np.int64)
    uniq, idx = np.unique(seg, return_inverse=True)
    idx = idx.reshape(-1)
    adj = mutual_adjacency(conn, uniq)
    seg_masks = segment_masks(masks, idx, len(uniq))
    cols, src, parts = [], [], []
    for j, row in enumerate(seg_masks):
        label = components(row, adj)
        for root in np.unique(label[label >= 0]):          # ascending: the part's smallest segment index
            part = np.nonzero(label == root)[0]
            parts.append(part)
            cols.append(np.isin(idx, part))
            src.append(j)
    out = np.stack(cols, 1) if cols else np.zeros((len(seg), 0), bool)
    return out, np.array(src, np.int64), parts, uniq

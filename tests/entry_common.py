"""Shared by the entry-node tests (test_entry_cut_host.py, test_gpu_entry_nodes.py): a scene's pair
array walked on the host -- every node is named `src` = pair << 1 | side, the record and side that
hold its box -- and the checks a cut table and a tile's entry record must pass."""
import numpy as np

LEAF = 0xffffffff


class Tree:
    """The sibling-pair array ([n, 16] u32: lb, rb, lcount, lfirst, rcount, rfirst) as a tree."""

    def __init__(self, pairs, n_tri):
        self.pairs = pairs
        n = len(pairs)
        count = pairs[:, [12, 14]].astype(np.int64)                 # [record, side]
        first = pairs[:, [13, 15]].astype(np.int64)
        self.count, self.first = count, first
        # the record that holds a record's parent node (record 0: the root's children, no parent)
        self.parent_src = np.full(n, -1, np.int64)
        inner = count == 0
        rec, side = np.nonzero(inner)
        self.parent_src[first[rec, side]] = rec * 2 + side
        # leaf slot -> the leaf's src
        self.leaf_of_slot = np.full(n_tri, -1, np.int64)
        rec, side = np.nonzero(~inner)
        for r, s in zip(rec, side):
            self.leaf_of_slot[first[r, s]:first[r, s] + count[r, s]] = r * 2 + s

    def child_record(self, src):
        r, s = src >> 1, src & 1
        return LEAF if self.count[r, s] else int(self.first[r, s])

    def ancestors(self, src):
        """src, its parent, ... up to a child of the root."""
        out = [int(src)]
        while self.parent_src[out[-1] >> 1] >= 0:
            out.append(int(self.parent_src[out[-1] >> 1]))
        return out

    def record_ancestors(self, rec):
        """rec, the record of its parent node, ..., record 0."""
        out = [int(rec)]
        while self.parent_src[out[-1]] >= 0:
            out.append(int(self.parent_src[out[-1]]) >> 1)
        return out

    def preorder(self):
        """Every node's src in depth-first order, left before right (iterative)."""
        out, stack = [], [1, 0]
        while stack:
            src = stack.pop()
            out.append(src)
            c = self.child_record(src)
            if c != LEAF:
                stack += [2 * c + 1, 2 * c]
        return out


def check_cut(tree, cut):
    """Every root-to-leaf path meets the cut exactly once; the cut is in depth-first order; lca[i][j]
    is the brute-force LCA's children record for every pair."""
    order = tree.preorder()
    pos = {src: k for k, src in enumerate(order)}
    cut_src = [int(x) for x in cut.src]
    assert len(set(cut_src)) == cut.n
    where = [pos[s] for s in cut_src]
    assert where == sorted(where), "the cut is not in depth-first order"
    index = {s: k for k, s in enumerate(cut_src)}
    # cut nodes on the path of every leaf: walk down, counting
    met = {1: 0, 0: 0}
    for src in order:
        up = met[src]
        here = up + (1 if src in index else 0)
        c = tree.child_record(src)
        if c == LEAF:
            assert here == 1, f"a path with {here} cut nodes"
        else:
            met[2 * c] = met[2 * c + 1] = here
    for k, s in enumerate(cut_src):
        assert int(cut.child[k]) == tree.child_record(s)
    chains = [tree.ancestors(s)[::-1] for s in cut_src]              # from a child of the root down to the node
    for i in range(cut.n):
        for j in range(cut.n):
            a, b = chains[i], chains[j]
            d = 0
            while d < len(a) and d < len(b) and a[d] == b[d]:
                d += 1
            if i == j:                                               # the node itself; a leaf enters at its parent's record
                c = tree.child_record(cut_src[i])
                want, depth = (c, d) if c != LEAF else (cut_src[i] >> 1, d - 1)
            else:
                want, depth = (0, 0) if d == 0 else (tree.child_record(a[d - 1]), d)
            assert int(cut.lca[i, j]) == want, (i, j)
            assert int(cut.depth[i, j]) == depth, (i, j)
    return index


def cut_above(tree, index, src):
    """The cut node (its number) on the path of node src."""
    for a in tree.ancestors(src):
        if a in index:
            return index[a]
    raise AssertionError("no cut node above a leaf")


def tile_sets(rects, W, H):
    """reach[tile row, tile column, k]: rectangle k has a pixel of the tile."""
    tx, ty = (W + 7) // 8, (H + 7) // 8
    a = 8 * np.arange(tx)
    b = np.minimum(a + 7, W - 1)
    p = 8 * np.arange(ty)
    q = np.minimum(p + 7, H - 1)
    r = rects.astype(np.int64)
    cols = np.maximum(a[:, None], r[None, :, 0]) <= np.minimum(b[:, None], r[None, :, 1])     # [tx, 64]
    rows = np.maximum(p[:, None], r[None, :, 2]) <= np.minimum(q[:, None], r[None, :, 3])     # [ty, 64]
    return rows[:, None, :] & cols[None, :, :]

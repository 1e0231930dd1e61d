"""algebra/merkle.rs restated literally on hashlib.sha3_256, and Celestia::commit / Celestia::verify (das/celestia.rs:73-169) over it: the
model of tests/test_gpu_das.py.  Leaves are `bytes`; a symbol of a square is the one-byte leaf bytes([e]) (celestia.rs:52).  Shares no
code with tests/merkle_model.py or the oracle.

The reference's `open` does not terminate on a one-leaf slice (mid = 0 sends the same slice down again, merkle.rs:36-45); here it
returns None there.  Its `verify` takes left / right from the bits of the index, which is the tree's shape only when every split is
even -- on a ragged tree it can reject the reference's own path.  `verify` below is that function as written; `verify_shaped` follows
the splits of `commit` instead and accepts exactly the paths that authenticate the leaf."""
import hashlib


def hash_(data):                                   # merkle.rs:8-12
    return hashlib.sha3_256(data).digest()


def commit(leafs):                                 # merkle.rs:15-25
    if len(leafs) == 1:
        return bytes(leafs[0])
    mid = len(leafs) // 2
    return hash_(commit(leafs[:mid]) + commit(leafs[mid:]))


def open_(index, leafs):                           # merkle.rs:28-46; None: the recursion would not end
    if len(leafs) == 2:
        return [bytes(leafs[1 - index])]
    if len(leafs) < 2:
        return None
    mid = len(leafs) // 2
    if index < mid:
        path = open_(index, leafs[:mid])
        other = leafs[mid:]
    else:
        path = open_(index - mid, leafs[mid:])
        other = leafs[:mid]
    if path is None:
        return None
    path.append(commit(other))
    return path


def verify(root, index, path, leaf):               # merkle.rs:49-66
    if len(path) == 1:
        if index == 0:
            return root == hash_(leaf + path[0])
        return root == hash_(path[0] + leaf)
    nxt = hash_(leaf + path[0]) if index % 2 == 0 else hash_(path[0] + leaf)
    return verify(root, index >> 1, path[1:], nxt)


def verify_shaped(root, index, n, path, leaf):
    """the path of leaf `index` of an n-leaf tree checked along the splits commit makes (mid = len / 2), whatever the index bits say"""
    sides = []                                     # from the root down: True = the leaf is in the right half
    lo, size = 0, n
    while size > 2:
        mid = size // 2
        right = index - lo >= mid
        sides.append(right)
        if right:
            lo, size = lo + mid, size - mid
        else:
            size = mid
        if size == 1:
            return False                           # a one-leaf slice: there is no path
    if size != 2 or len(path) != len(sides) + 1:
        return False
    acc = hash_(leaf + path[0]) if index - lo == 0 else hash_(path[0] + leaf)
    for right, sib in zip(reversed(sides), path[1:]):
        acc = hash_(sib + acc) if right else hash_(acc + sib)
    return acc == root


def celestia_commit(matrix):
    """Celestia::commit (celestia.rs:73-113) of a matrix of symbols (rows of ints): (row_roots, col_roots, data_root)"""
    rows = [[bytes([e]) for e in row] for row in matrix]
    row_roots = [commit(r) for r in rows]
    col_roots = [commit([r[i] for r in rows]) for i in range(len(rows[0]))]
    return row_roots, col_roots, commit(row_roots + col_roots)


def celestia_open(matrix, row, col, is_row):       # the proof half of Celestia::verify (:124-135)
    if is_row:
        return open_(col, [bytes([e]) for e in matrix[row]])
    return open_(row, [bytes([r[col]]) for r in matrix])


def celestia_verify(matrix, commitment, row, col, is_row):      # Celestia::verify (:115-169); None: its open does not terminate
    row_roots, col_roots, _ = commitment
    path = celestia_open(matrix, row, col, is_row)
    if path is None:
        return None
    leaf = bytes([matrix[row][col]])
    if is_row:
        return verify(row_roots[row], col, path, leaf)
    return verify(col_roots[col], row, path, leaf)


# ---- the item form the device computes (mzk_das_plan.h), derived here on its own ----------------------------------------------------
def item_sizes(n):
    """sizes (1 or 2) of the 2^floor(log2 n) bottom subtrees of an n-leaf tree, left to right: floor(log2 n) splits at mid = len / 2"""
    sizes = [n]
    for _ in range(n.bit_length() - 1):
        sizes = [h for s in sizes for h in (s // 2, s - s // 2)]
    assert len(sizes) == 1 << (n.bit_length() - 1) and set(sizes) <= {1, 2}
    return sizes


def commit_items(leafs):
    """the same root from the item form: items, then a full binary tree"""
    sizes = item_sizes(len(leafs))
    level, at = [], 0
    for s in sizes:
        level.append(bytes(leafs[at]) if s == 1 else hash_(bytes(leafs[at]) + bytes(leafs[at + 1])))
        at += s
    while len(level) > 1:
        level = [hash_(level[i] + level[i + 1]) for i in range(0, len(level), 2)]
    return level[0], sizes


def nonterminating(n):
    """indices whose leaf is a one-leaf LEFT item beside a two-leaf right item"""
    sizes = item_sizes(n)
    out, at = set(), 0
    for p, s in enumerate(sizes):
        if s == 1 and sizes[p ^ 1] == 2:
            assert p % 2 == 0
            out.add(at)
        at += s
    return out

"""tests/das_model.py against the reference's own test and against itself: test_celestia (das/celestia.rs:196-231) over the 2D code of
tests/rs_model.py, and for every leaf count 2 .. 255 the item form the device computes against the literal recursion.  CPU only."""
import random
import das_model as M
import rs_model as R


def _setup(chunk_size, expansion_factor, _data_size):      # Celestia::setup (celestia.rs:34-41): chunk_size * ceil(expansion_factor)
    import math
    return int(chunk_size * math.ceil(expansion_factor)), chunk_size


def test_celestia_as_the_reference_runs_it():
    codeword_size, _ = _setup(8, 2.0, 64)
    assert codeword_size == 16
    data = list(range(64))
    rs = R.setup_rs2d(codeword_size, codeword_size, len(data))
    encoded = R.encode_rs2d(data, rs)
    assert len(encoded) == 16 and all(len(r) == 16 for r in encoded)
    commitment = M.celestia_commit(encoded)
    assert len(commitment[0]) == 16 and len(commitment[1]) == 16 and len(commitment[2]) == 32
    for i in range(10):
        assert M.celestia_verify(encoded, commitment, i // 12, i % 12, False) is True
    assert R.decode_rs2d(encoded, rs)[:63] == data[:63]
    mal = R.encode_rs2d(list(range(1, 65)), rs)
    assert M.celestia_verify(mal, commitment, 0, 0, False) is False
    # rows too, and the row / column roots are not interchangeable
    assert all(M.celestia_verify(encoded, commitment, r, c, True) for r in range(16) for c in range(16))
    assert commitment[0] != commitment[1]


def test_merkle_as_the_reference_tests_it():                # merkle.rs:73-91
    leafs = [b"leaf1", b"leaf2", b"leaf3", b"leaf4"]
    root = M.commit(leafs)
    proof = M.open_(2, leafs)
    assert M.verify(root, 2, proof, leafs[2]) and not M.verify(root, 2, proof, leafs[3])
    assert M.commit([b"x"]) == b"x"


def test_item_form_equals_the_recursion_for_every_leaf_count():
    rnd = random.Random(20)
    for n in range(2, 256):
        leafs = [bytes([rnd.randrange(256)]) for _ in range(n)]
        root = M.commit(leafs)
        from_items, sizes = M.commit_items(leafs)
        assert from_items == root and len(root) == 32, n
        assert len(sizes) == 1 << (n.bit_length() - 1) and sum(sizes) == n, n
        # 32-byte leaves (the data-root tree) as well
        wide = [bytes(rnd.randrange(256) for _ in range(32)) for _ in range(2 * n)]
        assert M.commit_items(wide)[0] == M.commit(wide), n


def test_nonterminating_indices_are_the_one_leaf_left_items_beside_two_leaf_items():
    for n in range(2, 256):
        leafs = [bytes([(7 * i + n) & 255]) for i in range(n)]
        root = M.commit(leafs)
        paths = [M.open_(i, leafs) for i in range(n)]
        assert {i for i, p in enumerate(paths) if p is None} == M.nonterminating(n), n
        d = n.bit_length() - 1
        for i, p in enumerate(paths):
            if p is None:
                continue
            assert len(p) in (d, d + 1) and len(p[0]) == 1 and all(len(e) in (1, 32) for e in p), (n, i)
            assert M.verify_shaped(root, i, n, p, leafs[i]), (n, i)
            assert not M.verify_shaped(root, i, n, p, bytes([leafs[i][0] ^ 1])), (n, i)
            if n & (n - 1) == 0:                            # the reference's verify reads the shape off the index bits: right for even splits only
                assert M.verify(root, i, p, leafs[i]), (n, i)

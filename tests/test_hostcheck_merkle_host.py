"""Merkle::hash and Merkle::verify of the C++ mirror (myzkp_amd/host/myzkp.hpp) are plain host code over a small SHA3-256 of the
header's own.  tests/hostcheck/merkle_host_shim.cpp, a stand-alone program with its own main that links nothing of the library, runs
them on vectors written here by tests/das_model.py: built once plain and once with -fsanitize=address,undefined.  CPU only."""
import os, random, subprocess
import das_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


def _vectors():
    rnd = random.Random(9)
    lines = []
    for n in [0, 1, 2, 3, 32, 33, 64, 65, 134, 135, 136, 137, 200, 271, 272, 273, 500]:      # around one and two blocks of the 136-byte rate
        msg = bytes(rnd.randrange(256) for _ in range(n))
        lines.append("H %s %s" % (msg.hex() or "-", M.hash_(msg).hex()))
    accepted = rejected = 0
    for n in [2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 33, 64, 255]:
        leafs = [bytes([rnd.randrange(256)]) for _ in range(n)]
        root = M.commit(leafs)
        for i in range(n):
            path = M.open_(i, leafs)
            if path is None:
                continue
            for leaf in (leafs[i], bytes([leafs[i][0] ^ 0x80])):
                want = M.verify(root, i, path, leaf)           # the reference's verify as written: it rejects most paths of a ragged tree
                accepted += want
                rejected += not want
                lines.append("V %s %d %s %d %s" % (root.hex(), i, leaf.hex(), want, " ".join(e.hex() for e in path)))
    # wide leaves: the reference's own test (merkle.rs:73-91)
    leafs = [b"leaf1", b"leaf2", b"leaf3", b"leaf4"]
    root, path = M.commit(leafs), M.open_(2, leafs)
    lines.append("V %s 2 %s 1 %s" % (root.hex(), leafs[2].hex(), " ".join(e.hex() for e in path)))
    lines.append("V %s 2 %s 0 %s" % (root.hex(), leafs[3].hex(), " ".join(e.hex() for e in path)))
    assert accepted > 100 and rejected > 100
    return lines


def test_mirror_hash_and_verify_equal_the_model(tmp_path):
    src = os.path.join(HERE, "hostcheck", "merkle_host_shim.cpp")
    vec = tmp_path / "vectors.txt"
    lines = _vectors()
    vec.write_text("\n".join(lines) + "\n")
    common = ["g++", "-std=c++17", "-Wall"]
    plain, san = str(tmp_path / "merkle_host_shim"), str(tmp_path / "merkle_host_shim_san")
    subprocess.check_call(common + ["-O1", "-o", plain, src])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    want = "ok %d %d\n" % (sum(l[0] == "H" for l in lines), sum(l[0] == "V" for l in lines))
    for exe in (plain, san):
        r = subprocess.run([exe, str(vec)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.stdout == want

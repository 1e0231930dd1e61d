"""The host parameters of interpolation and zerofier over a prefix of a power-of-two subgroup (myzkp_amd/csrc/mzk_prefix_plan.h:
prefix_candidate, prefix_system_inverse, prefix_zerofier_params) run by tests/hostcheck/prefix_plan_shim.cpp, a stand-alone program
built with -fsanitize=address,undefined, against Python integers: M128 and Fr, subgroups of N = 4, 8, 64, 1024 points of which
m = 0, 1, 3, 7, 64 are missing.  Ainv times A[t][j] = x_(n+j)^(1+t) is the identity; (rho_j, w_j) are the closed form of
tests/test_prefix_math.py, which shows that those closed forms give the interpolant and the zerofier; prefix_candidate takes the
prefix and refuses a domain that does not start at 1, a generator of half or twice the order, a wrong third or last point, more than
64 missing points and fewer than two points.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FR, M128 = 0, 1
P = {FR: 21888242871839275222246405745257275088548364400416034343698204186575808495617, M128: 1 + 407 * (1 << 119)}
SHAPES = [(N, m) for N in (4, 8, 64, 1024) for m in (0, 1, 3, 7, 64) if m < N - 1]


def root(fid, lg):
    p = P[fid]
    if fid == FR:
        return pow(pow(5, (p - 1) >> 28, p), 1 << (28 - lg), p)
    return pow(85408008396924667383611388730472331217, 1 << (119 - lg), p)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("prefix_plan")
    exe = str(d / "prefix_plan_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "prefix_plan_shim.cpp")])

    def run(fid, ops):
        """ops: tuples (name, int ...) -> one output line each, as lists of words"""
        path = str(d / ("ops_%d.txt" % fid))
        with open(path, "w") as f:
            for op in ops:
                f.write(" ".join([op[0]] + ["%x" % v for v in op[1:]]) + "\n")
        r = subprocess.run([exe, str(fid), path], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.split("\n")[:-1]
        assert lines[-1] == "ok" and len(lines) == len(ops) + 1, r.stdout[-3000:]
        return [l.split() for l in lines[:-1]]
    return run


@pytest.mark.parametrize("fid", [M128, FR])
def test_system_inverse_and_zerofier_parameters(shim, fid):
    p = P[fid]
    ops = []
    for N, m in SHAPES:
        g = root(fid, N.bit_length() - 1)
        ops += [("inverse", g, N - m, m), ("zerofier", g, N - m, N)]
    got = shim(fid, ops)
    for k, (N, m) in enumerate(SHAPES):
        n = N - m
        g = root(fid, N.bit_length() - 1)
        miss = [pow(g, n + j, p) for j in range(m)]
        ainv = [int(w, 16) for w in got[2 * k]]
        assert len(ainv) == m * m, (N, m)
        A = [[pow(x, 1 + t, p) for x in miss] for t in range(m)]
        for j in range(m):
            row = ainv[j * m:(j + 1) * m]
            assert [sum(row[t] * A[t][c] for t in range(m)) % p for c in range(m)] == [int(c == j) for c in range(m)], (N, m, j)
        params = [int(w, 16) for w in got[2 * k + 1]]
        want = []
        for j in range(m):
            den = 1
            for l in range(m):
                if l != j:
                    den = den * (miss[j] - miss[l]) % p
            want += [pow(den, -1, p), pow(miss[j], -1, p)]
        assert params == want, (N, m)


@pytest.mark.parametrize("fid", [M128, FR])
def test_prefix_candidate_takes_the_prefix_and_nothing_else(shim, fid):
    p = P[fid]
    ops, want = [], []

    def case(domain, verdict):
        ops.append(("candidate", len(domain)) + tuple(domain))
        want.append(verdict)

    for N, m in SHAPES:
        n, lg = N - m, N.bit_length() - 1
        g = root(fid, lg)
        dom = [pow(g, i, p) for i in range(n)]
        case(dom, ["1", str(N)])
        case([2] + dom[1:], ["0"])                                            # does not start at 1
        if n > 2:
            half, twice = root(fid, lg - 1), root(fid, lg + 1)
            case([pow(half, i, p) for i in range(n)], ["0"])                  # a generator of order N / 2 ...
            case([pow(twice, i, p) for i in range(n)], ["0"])                 # ... and of 2 N: every point a power of domain[1]
            case(dom[:2] + [(dom[2] + 1) % p] + dom[3:], ["0"])               # the third point
            if n > 3:
                case(dom[:-1] + [(dom[-1] + 1) % p], ["0"])                   # the last point
                case(dom[:-1] + [dom[-2]], ["0"])
    # 64 missing points are taken, 65 are not
    g = root(fid, 8)
    case([pow(g, i, p) for i in range(256 - 64)], ["1", "256"])
    case([pow(g, i, p) for i in range(256 - 65)], ["0"])
    # fewer than two points
    case([], ["0"])
    case([1], ["0"])
    case([1, p - 1], ["1", "2"])
    assert shim(fid, ops) == want

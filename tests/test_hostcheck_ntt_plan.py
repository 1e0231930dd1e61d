"""The transforms' launch schedule (ntt_plan in myzkp_amd/csrc/mzk_ntt_plan.h: tile geometry, the split of log2 n into passes, and per
pass the grid, block, LDS bytes and write-through flag that mzk_ntt.hip and mzk_gl.hip launch) run on the host by
tests/hostcheck/ntt_plan_shim.cpp, a stand-alone program built with -fsanitize=address,undefined: all four fields, every log2 n the
entry points admit, batches of 1, 2, 3, 16 and the largest admitted (2^40 / n), under the default switches and, for Fr and M128, with the
large geometry forced from 2^14 .. 2^32 and the two-workgroup M128 geometry from 2^20, 2^21 or never.  Checked here in integers: what
the kernels rely on without checking it themselves, the LDS bytes, the write-through window, and the schedule written out below.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FR, M128, M64, M64X3 = 0, 1, 3, 4
MAX_LOG = {FR: 28, M128: 32, M64: 32, M64X3: 32}            # field_max_log; the two-adicity of Goldilocks
ELEM_BYTES = {FR: 32, M128: 16, M64: 8, M64X3: 24}
NC = {FR: 1, M128: 1, M64: 1, M64X3: 3}                     # workgroups per tile: one per coefficient
LIMBS = {FR: 9, M128: 5}                                    # 29-bit limbs of an element in LDS
WORDS = {FR: 8, M128: 4}                                    # packed 32-bit words of an element
S, S1, L, M, GL = range(5)
GEO = {S: (10, 256, 8, 0, 1), S1: (10, 256, 10, 0, 1), L: (12, 1024, 10, 0, 1), M: (12, 512, 10, 1, 4), GL: (12, 256, 8, 0, 3)}  # tl, threads, widest level, no twiddles in LDS, waves per SIMD
STRIDED, LAST = 0, 1
DEFAULT = -2


def batches(logn):
    return (1, 2, 3, 16, (1 << 40) >> logn)


def cases():
    out = []
    for fid in (FR, M128, M64, M64X3):
        for logn in range(1, MAX_LOG[fid] + 1):
            for b in batches(logn):
                out.append((fid, logn, b, DEFAULT, DEFAULT, DEFAULT))
                if fid in (FR, M128):
                    for force in range(14, 33):
                        for twg in (20, 21, 99):
                            out.append((fid, logn, b, force, force, twg))
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{case: dict(err, geo, large, lg, tmp, attr, steps=[dict, ...])}, geometries, default knobs"""
    d = tmp_path_factory.mktemp("ntt_plan")
    exe = str(d / "ntt_plan_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "ntt_plan_shim.cpp")])
    cs = cases()
    src = str(d / "cases.txt")
    with open(src, "w") as f:
        f.write("".join("%d %d %d %d %d %d\n" % c for c in cs))
    r = subprocess.run([exe, src], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cs)
    knobs = tuple(map(int, lines[-2].split()[1:]))
    assert lines[-2].split()[0] == "K"
    geos = {}
    for ln in lines[-7:-2]:
        f = ln.split()
        assert f[0] == "G"
        geos[int(f[1])] = tuple(map(int, f[2:]))
    out = {}
    for ln in lines[:-7]:
        f = ln.split()
        assert f[0] == "P"
        v = list(map(int, f[1:]))
        case, (err, geo, large, nlev), lg, (tmp, attr, ns), rest = tuple(v[:6]), v[6:10], v[10:14], v[14:17], v[17:]
        assert len(rest) == 11 * ns
        steps = [dict(zip(("kind", "lgn", "lgM", "lgc", "lgr", "lg_rows", "total_rows", "grid", "block", "lds", "wt"), rest[11 * i:11 * i + 11])) for i in range(ns)]
        assert all(x == 0 for x in lg[nlev:])
        out[case] = dict(err=err, geo=geo, large=large, lg=tuple(lg[:nlev]), tmp=tmp, attr=attr, steps=steps)
    assert len(out) == len(cs)
    return out, geos, knobs


def test_geometries_and_default_switches(plans):
    _, geos, knobs = plans
    assert geos == GEO
    assert knobs == (-1, -1, 21, 21, 24, 26, 3)      # force-large-from Fr, M128; M128 two-workgroups-from; write-through low, high Fr, high M128, mask


def lds_bytes(fid, geo):
    """Geo::lds_bytes of mzk_ntt.hip: the tile limb-major, then the widest level's n/2 in-tile twiddles, one row per limb -- or per packed
    word where limbs would not fit 160 KiB -- and none where the geometry reads them from memory"""
    tl, _, maxlv, twg, _ = GEO[geo]
    tile, tws = 1 << tl, 1 << (maxlv - 1)
    if twg:
        return 4 * LIMBS[fid] * tile
    packed = 4 * LIMBS[fid] * (tile + tws) > 160 * 1024
    return 4 * (LIMBS[fid] * tile + (WORDS[fid] if packed else LIMBS[fid]) * tws)


def test_lds_bytes_of_the_widest_level():
    assert lds_bytes(FR, S) == 41472 and lds_bytes(FR, S1) == 55296 and lds_bytes(FR, L) == 163840 == 160 * 1024
    assert lds_bytes(M128, L) == 92160 and lds_bytes(M128, M) == 81920


def test_what_the_kernels_rely_on(plans):
    plans, _, _ = plans
    for (fid, logn, batch, force, _, twg), p in plans.items():
        where = (fid, logn, batch, force, twg, p)
        gl = fid in (M64, M64X3)
        assert p["err"] == 0, where                      # nothing admitted is refused: "too many tiles", "block smaller than a tile"
        tl, threads, maxlv, _, _ = GEO[p["geo"]]
        lg, steps = p["lg"], p["steps"]
        assert 1 <= len(lg) <= 4 and sum(lg) == logn and len(steps) == len(lg), where
        assert (p["geo"] == GL) == gl and (p["geo"] in (L, M)) == bool(p["large"]), where
        assert p["geo"] != M or fid == M128, where      # the only field with kernels of that geometry
        if len(lg) == 1:
            assert lg[0] <= tl and p["geo"] in (S, S1, GL), where
            assert p["geo"] != S or lg[0] <= maxlv, where
        else:
            assert all(x <= maxlv for x in lg) and p["geo"] != S1, where      # S1 has no strided kernels
        assert [s["kind"] for s in steps] == [STRIDED] * (len(lg) - 1) + [LAST], where
        assert [s["lgn"] for s in steps] == list(lg), where
        data_bytes = (batch << logn) * ELEM_BYTES[fid]
        want_lds = 0 if gl else lds_bytes(fid, p["geo"])
        lg_after = logn
        for s in steps:
            assert 1 <= s["grid"] < 1 << 31 and s["block"] == threads, where
            assert s["lds"] == want_lds <= 160 * 1024 and (s["lds"] <= 64 * 1024) == (not p["attr"]), where
            if s["kind"] == STRIDED:
                assert s["lgn"] >= 2 and s["lgn"] + s["lgc"] == tl and s["lgM"] >= s["lgc"] >= 0 and logn >= tl, where
                assert s["lgM"] == lg_after - s["lgn"], where
                assert s["grid"] == (batch << (logn - tl)) * NC[fid], where
                lg_after = s["lgM"]
            else:
                assert s["lgn"] == lg_after and s["lg_rows"] == logn - s["lgn"] and s["total_rows"] == batch << s["lg_rows"], where
                want_lgr = max([r for r in range(tl - s["lgn"] + 1) if 1 << r <= s["total_rows"]] or [0])
                assert s["lgr"] == want_lgr, where
                tiles, rem = divmod(s["grid"], NC[fid])
                assert rem == 0 and tiles << s["lgr"] >= s["total_rows"] > (tiles - 1) << s["lgr"], where      # covers the rows; no idle workgroup
        # write-through window and the temporary
        hi = {FR: 24, M128: 26}.get(fid)
        want_wt = not gl and len(lg) > 1 and 1 << 21 <= data_bytes <= 1 << hi
        assert all(s["wt"] == int(want_wt) for s in steps), where
        assert p["tmp"] == (data_bytes if len(lg) > 1 else 0), where


def test_forced_large_geometry(plans):
    plans, _, _ = plans
    for (fid, logn, batch, force, _, twg), p in plans.items():
        if force == DEFAULT:
            continue
        large = logn >= max(force, 14)
        assert p["large"] == int(large), (fid, logn, batch, force, twg)
        assert p["geo"] == ((M if fid == M128 and logn >= twg else L) if large else S1 if logn in (9, 10) else S), (fid, logn, batch, force, twg)
        if large:
            assert len(p["lg"]) == -(-logn // 10), (fid, logn, batch, force, twg)


# The schedule under the default switches: levels in launch order.  Fr / M128 use (levels, geometry); "LM" is L for Fr, and for M128
# L at 2^20 and M from 2^21 on (two-workgroups-from = 21).
FIELD_TO_19 = {**{k: ((k,), S) for k in range(1, 9)}, 9: ((9,), S1), 10: ((10,), S1), 11: ((6, 5), S), 12: ((6, 6), S), 13: ((7, 6), S), 14: ((7, 7), S),
               15: ((8, 7), S), 16: ((8, 8), S), 17: ((6, 6, 5), S), 18: ((6, 6, 6), S), 19: ((7, 6, 6), S)}
GL_TO_19 = {**{k: (k,) for k in range(1, 13)}, 13: (6, 7), 14: (7, 7), 15: (7, 8), 16: (8, 8), 17: (5, 6, 6), 18: (6, 6, 6), 19: (6, 6, 7)}
# log2 n: (small batch, large batch, Goldilocks); small batch: at most 2 transforms for Fr, 1 for M128
FROM_20 = {
    20: (((10, 10), "LM"), ((7, 7, 6), S), (6, 7, 7)),
    21: (((7, 7, 7), S), ((7, 7, 7), S), (7, 7, 7)),
    22: (((8, 7, 7), S), ((8, 7, 7), S), (7, 7, 8)),
    23: (((8, 8, 7), S), ((8, 8, 7), S), (7, 8, 8)),
    24: (((8, 8, 8), S), ((8, 8, 8), S), (8, 8, 8)),
    25: (((9, 8, 8), "LM"), ((7, 6, 6, 6), S), (6, 6, 6, 7)),
    26: (((9, 9, 8), "LM"), ((7, 7, 6, 6), S), (6, 6, 7, 7)),
    27: (((9, 9, 9), "LM"), ((7, 7, 7, 6), S), (6, 7, 7, 7)),
    28: (((10, 9, 9), "LM"), ((7, 7, 7, 7), S), (7, 7, 7, 7)),
    29: (((10, 10, 9), "LM"), ((8, 7, 7, 7), S), (7, 7, 7, 8)),
    30: (((10, 10, 10), "LM"), ((8, 8, 7, 7), S), (7, 7, 8, 8)),
    31: (((8, 8, 8, 7), S), ((8, 8, 8, 7), S), (7, 8, 8, 8)),
    32: (((8, 8, 8, 8), S), ((8, 8, 8, 8), S), (8, 8, 8, 8)),
}


def test_default_schedule_is_the_pinned_table(plans):
    plans, _, _ = plans
    seen = 0
    for fid in (FR, M128, M64, M64X3):
        for logn in range(1, MAX_LOG[fid] + 1):
            for b in batches(logn):
                p = plans[(fid, logn, b, DEFAULT, DEFAULT, DEFAULT)]
                where = (fid, logn, b, p)
                seen += 1
                if fid in (M64, M64X3):
                    assert p["lg"] == (GL_TO_19[logn] if logn < 20 else FROM_20[logn][2]) and p["geo"] == GL, where
                    continue
                if logn < 20:
                    lg, geo = FIELD_TO_19[logn]
                else:
                    small = b <= (2 if fid == FR else 1)
                    lg, geo = FROM_20[logn][0 if small else 1]
                    if geo == "LM":
                        geo = L if fid == FR or logn < 21 else M
                assert (p["lg"], p["geo"]) == (lg, geo), where
    assert seen == 5 * (28 + 3 * 32)

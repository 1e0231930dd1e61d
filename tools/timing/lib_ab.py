"""Same-box A/B of two builds of the library under `python bench.py`: the runs of build A (MZK_HIP_LIB = its .so, e.g. one built from
the parent commit in another worktree) and of this tree's build alternate, ROUNDS times; the shader clock (hwmon freq1_input, highest
reading taken every 20 ms) is sampled while each run is going.  Prints one line per run and the medians, min, max and spread:
    python tools/timing/lib_ab.py PARENT_LIB.so ROUNDS [bench.py arguments, e.g. --full --skip-cpu]
Stops at the first run that fails (nothing more is started on a device a run has failed on)."""
import glob, json, os, subprocess, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KEEP = ("ms_per_step", "value", "msm_2p20_pairs_per_s", "msm_2p24_pairs_per_s", "msm_2p24_ms", "ntt_2p20_elems_per_s", "ntt_2p24_elems_per_s", "legs_ms")


def sclk_mhz():
    v = []
    for f in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input"):
        try:
            v.append(int(open(f).read()) // 1000000)
        except Exception:
            pass
    return max(v) if v else None


def one_run(lib, extra):
    env = dict(os.environ)
    if lib:
        env["MZK_HIP_LIB"] = lib
    samples, stop = [], threading.Event()

    def sampler():
        while not stop.is_set():
            c = sclk_mhz()
            if c:
                samples.append(c)
            time.sleep(0.02)
    th = threading.Thread(target=sampler)
    th.start()
    p = subprocess.run([sys.executable, "bench.py"] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    stop.set()
    th.join()
    if p.returncode != 0:
        sys.exit("bench.py failed (%d): %s" % (p.returncode, p.stderr[-1500:]))
    return json.loads(p.stdout.strip().splitlines()[-1]), (max(samples) if samples else None)


if __name__ == "__main__":
    parent, rounds, extra = os.path.abspath(sys.argv[1]), int(sys.argv[2]), sys.argv[3:]
    res = {"parent": [], "change": []}
    for r in range(rounds):
        for tag in ("parent", "change"):
            line, clk = one_run(parent if tag == "parent" else None, extra)
            res[tag].append(line["ms_per_step"])
            print("round %d %-6s %s sclk_max_mhz_while_running=%s" % (r, tag, json.dumps({k: line[k] for k in KEEP if k in line}), clk), flush=True)
    for tag, v in res.items():
        s = sorted(v)
        med = s[len(s) // 2] if len(s) % 2 else (s[len(s) // 2 - 1] + s[len(s) // 2]) / 2
        print("%-6s ms_per_step n=%d median %.4f min %.4f max %.4f spread %.4f" % (tag, len(s), med, s[0], s[-1], s[-1] - s[0]))

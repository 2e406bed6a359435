"""A/B of the pooled-row last block against the full block, alternating in one session on one GPU:
every step is a fresh child process with MMR_FULL_LAST_BLOCK=1 or 0 under its own time limit; the first failure stops the run.

    python tools/ab_last_block.py PLAN [OUT_DIR]

PLAN: headline = bench.py cfg2, 5 runs per side, 200 steps, outputs of the first pair compared array for array;
      others   = cfg3 and cfg5, 3 runs per side; trace = rocprofv3 --kernel-trace --stats of `bench.py --lanes 1`, both sides;
      small    = tools/time_small_batch.py (batch 1 / 10 / 32), both sides twice.
Writes ab_<cfg>.json, dump_<cfg>_same.json, trace_<side>/, small_<side>_<n>.json and a log under OUT_DIR (default ab_out/).
profiles/pooled_last_block.md is a digest of one such session."""
import json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "ab_out")
os.makedirs(OUT, exist_ok=True)
plan = sys.argv[1]
log = open(os.path.join(OUT, f"ab_{plan}.log"), "a")


def run(cmd, full, limit, tag):
    env = dict(os.environ, MMR_FULL_LAST_BLOCK="1" if full else "0")
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    msg = f"[{tag} full={int(full)}] rc={p.returncode} {time.time()-t0:.0f}s"
    print(msg, flush=True)
    log.write(msg + "\n" + p.stdout[-6000:] + "\n" + p.stderr[-3000:] + "\n"); log.flush()
    if p.returncode != 0:
        print(p.stdout[-1500:], p.stderr[-1500:])
        sys.exit(1)       # nothing more on the GPU after a failure
    return p.stdout


def bench_line(out):
    for ln in reversed(out.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit("no JSON line")


def alternate(cfg, runs, steps, warmup, dump):
    res = {"full": [], "pooled": []}
    for r in range(runs):
        for side in ("full", "pooled"):
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--config", cfg, "--steps", str(steps), "--warmup", str(warmup)]
            if dump and r == 0:
                cmd += ["--dump-outputs", os.path.join(OUT, f"dump_{cfg}_{side}")]
            j = bench_line(run(cmd, side == "full", 240, f"{cfg} run{r}"))
            res[side].append(j)
            print("   ", side, {k: j[k] for k in j if k in ("value", "ms_per_step", "metric", "unit")}, flush=True)
    json.dump(res, open(os.path.join(OUT, f"ab_{cfg}.json"), "w"), indent=1)
    if dump:
        same = {}
        for name in ("features", "topk_scores", "topk_ids"):
            a = find(os.path.join(OUT, f"dump_{cfg}_full"), name); b = find(os.path.join(OUT, f"dump_{cfg}_pooled"), name)
            same[name] = bool(a is not None and b is not None and a.shape == b.shape and a.tobytes() == b.tobytes())
        print(cfg, "dump-outputs identical:", same, flush=True)
        json.dump(same, open(os.path.join(OUT, f"dump_{cfg}_same.json"), "w"))


def find(d, name):
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            if f.startswith(name) and f.endswith(".npy"):
                return np.load(p)
            if f.endswith(".npz"):
                z = np.load(p)
                if name in z:
                    return z[name]
    return None


if plan == "headline":
    alternate("cfg2", 5, 200, 20, True)
elif plan == "others":
    alternate("cfg3", 3, 200, 20, True)
    alternate("cfg5", 3, 40, 5, True)
elif plan == "trace":
    for side in ("full", "pooled"):
        d = os.path.join(OUT, f"trace_{side}")
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "bench", "--output-format", "csv", "--",
             sys.executable, "bench.py", "--gpus", "1", "--lanes", "1"], side == "full", 300, "trace")
elif plan == "small":
    for r in range(2):
        for side in ("full", "pooled"):
            out = run([sys.executable, "tools/time_small_batch.py"], side == "full", 280, f"small run{r}")
            open(os.path.join(OUT, f"small_{side}_{r}.json"), "w").write(out[out.index("{"):])

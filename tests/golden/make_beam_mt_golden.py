"""Writes tests/golden/beam_mt_golden.json: the digests and counts of the float32 restatement (tests/beam_mt_ref.py) on the M2 and
M3 cases of tests/test_gpu_beam_mt.py, which are too slow to restate with every run of the suite (up to a minute each).
    python -m tests.golden.make_beam_mt_golden [processes [m2|m3]]      (with m2 or m3: those cases alone, the others kept)
Every case asserts here, on the CPU, what makes it worth running on the GPU (see the test file)."""
import json
import multiprocessing
import os
import sys
import time

from tests import beam_mt_ref as MR


def one(job):
    name, kind, W, K = job
    t0 = time.time()
    if name == "m2":
        c = MR.m2_case(kind)
        N, T, B, _ = MR.M2_SHAPE
        o = MR.case_ref(c, W, K, W, T, max_words=T)
    else:
        c = MR.m3_case(kind)
        N, T, B, K, W = MR.M3_SHAPE
        o = MR.case_ref(c, W, K, W, T, max_words=T)
    facts = MR.m2_facts(o["diags"])
    live = int((o["lengths"] >= 0).sum())
    entry = dict(sha=MR.digests(o), x=MR.input_digest(c), live=live, **facts)
    print(f"{name}/{kind}/W{W}/K{K}: {time.time() - t0:.0f} s, live {live}, {facts}", flush=True)
    return f"{name}/{kind}/W{W}/K{K}", entry


def main():
    jobs = [("m3", kind, MR.M3_SHAPE[4], MR.M3_SHAPE[3]) for kind in MR.KINDS]
    jobs += [("m2", kind, W, K) for W in sorted(MR.M2_W, reverse=True) for K in sorted(MR.M2_K, reverse=True) for kind in MR.KINDS]
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(8, os.cpu_count() or 1)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), MR.GOLDEN)
    out = {}
    if len(sys.argv) > 2:
        jobs = [j for j in jobs if j[0] == sys.argv[2]]
        with open(path) as f:
            out = {k: v for k, v in json.load(f).items() if not k.startswith(sys.argv[2] + "/")}
    with multiprocessing.Pool(procs) as pool:
        out.update(pool.imap_unordered(one, jobs))
    with open(path, "w") as f:
        json.dump(dict(sorted(out.items())), f, indent=1)
        f.write("\n")
    print("wrote", path, len(out), "cases")


if __name__ == "__main__":
    main()

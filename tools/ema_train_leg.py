"""optim(ms) of `bin/Train` on synthetic config-2 batches (the TDS-CTC recipe's train.cfg, batch 32, T = 1500) with and without
--slimIPL_ema=true: what the averaged teacher's one launch per update adds to the reference's optimizer timer (the last report =
the second half of the updates).   python tools/ema_train_leg.py [updates] [batch]"""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wav2letter_amd import recipes

updates = int(sys.argv[1]) if len(sys.argv) > 1 else 8
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
exe = os.path.join(ROOT, "wav2letter_amd", "bin", "Train")
with tempfile.TemporaryDirectory() as d:
    os.makedirs(os.path.join(d, "arch", "am_arch"))
    open(os.path.join(d, "arch", "am_arch", "am_tds_ctc.arch"), "w").write(recipes.tds_ctc_arch())
    os.makedirs(os.path.join(d, "am"))
    open(os.path.join(d, "am", "librispeech-train-all-unigram-10000.tokens"), "w").write("".join(f"tok{i}\n" for i in range(9997)))
    open(os.path.join(d, "train.cfg"), "w").write(recipes.tds_ctc_train_cfg())
    for tag, extra in (("plain", []), ("ema", ["--slimIPL_ema=true"]), ("plain again", []), ("ema again", ["--slimIPL_ema=true"])):
        cmd = [exe, "train", f"--flagsfile={os.path.join(d, 'train.cfg')}", f"--rundir={os.path.join(d, 'runs_' + tag.replace(' ', '_'))}",
               f"--archdir={os.path.join(d, 'arch')}", f"--tokensdir={os.path.join(d, 'am')}", f"--w2l_synth_updates={updates}",
               f"--reportiters={updates // 2}", "--w2l_synth_frames=1500", f"--batchsize={B}", "--w2l_synth_target_len=80", "--w2l_synth_pool=4"] + extra
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            print("[ema-train] " + json.dumps({"run": tag, "error": (p.stderr or p.stdout)[-400:]}), flush=True)
            sys.exit(1)
        row = [l for l in p.stdout.splitlines() if l.startswith("epoch:")][-1]
        kv = {k.strip(): v.strip() for k, v in (item.split(":", 1) for item in row.split(" | "))}
        print("[ema-train] " + json.dumps({"run": tag, "optim_ms": float(kv["optim(ms)"]), "bch_ms": float(kv["bch(ms)"]), "bwd_ms": float(kv["bwd(ms)"]),
                                           "loss": float(kv["loss"])}), flush=True)

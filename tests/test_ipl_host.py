"""The host state of slimIPL (include/fl_compat/ipl.h) against its Python twin (tests/ipl_ref.py): scripted runs decision by
decision, the cache file formats, the refusal of an unknown --slimIPL_type.  No device: plain g++."""
import os
import subprocess

import pytest

import ipl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ipl") / "ipl_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "ipl_test.cpp"), "-o", out], check=True)
    return out


def test_scripted_runs_decide_line_for_line_as_the_python_twin(exe):
    """H1: all four types, sup:unsup 1:3 and 0:1, 3 and 7 unsupervised batches, fixed_cache_updates 2 and 5, update probability
    0, 0.5 and 1, 40 steps each"""
    got = subprocess.run([exe, "scenarios"], capture_output=True, text=True, check=True).stdout.splitlines()
    want = []
    sc = ipl_ref.scenarios()
    assert {s[0] for s in sc} == set(ipl_ref.TYPES) and {s[1:3] for s in sc} == {(1, 3), (0, 1)} and {s[3] for s in sc} == {3, 7}
    assert {(s[4], s[5]) for s in sc if s[0] == "fixed-pre-cache"} == {(U, p) for U in (2, 5) for p in (0.0, 0.5, 1.0)}
    for type_, sup, unsup, n, U, prob, seed in sc:
        want.append(f"== {type_} {sup} {unsup} {n} {U} {prob:g}")
        lines = ipl_ref.scenario(type_, sup, unsup, n, U, prob, seed)
        assert sum(1 for l in lines if l.split()[1:2] in (["sup"], ["unsup"])) == 40
        want += lines
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)


def test_the_scripted_runs_show_what_each_mode_is_about():
    """the twin itself, read against recipes/slimIPL/src/Train.cpp: pre-cache and cache skip the update the first time a batch is
    seen and train on the labels of its last visit afterwards; cache relabels after the update (the ' mark), pre-cache before;
    fixed-pre-cache fills its cache first (no training batch, every step labels), then trains on cached batch indices only, and
    with update probability 0 never labels again; sup:unsup 0:1 takes no supervised step at all"""
    for type_ in ("cache", "pre-cache"):
        seen = {}
        for l in ipl_ref.scenario(type_, 1, 3, 3, 2, 1.0, 5):
            f = l.split()
            if len(f) < 3 or f[1] != "unsup":
                continue
            t, b = int(f[0]), int(f[2].split("=")[1])
            texts = l.split("texts=")[1].rsplit(" update=", 1)[0]
            if b not in seen:
                assert l.endswith("rows= texts= update=0"), l
            else:
                mark = "'" if type_ == "cache" else ""
                assert texts == f"w{b} x0 t{seen[b]}{mark};w{b} x1 t{seen[b]}{mark}" and l.endswith("update=1"), l
            seen[b] = t
        assert len(seen) == 3
    for U in (2, 5):
        lines = [l for l in ipl_ref.scenario("fixed-pre-cache", 0, 1, 7, U, 0.0, 9) if " unsup " in l]
        assert len(lines) == 40 and all("train=-1" in l and "relabel=1" in l and "update=0" in l for l in lines[:U])
        assert all("train=-1" not in l and "relabel=0 next=-1" in l and "update=1" in l for l in lines[U:])
        filled = {int(l.split("next=")[1].split()[0]) for l in lines[:U]}
        assert {int(l.split("train=")[1].split()[0]) for l in lines[U:]} == filled
    assert not any(l.endswith(" sup") for l in ipl_ref.scenario("naive", 0, 1, 3, 2, 1.0, 3))
    naive = [l for l in ipl_ref.scenario("naive", 1, 3, 3, 2, 1.0, 3) if " unsup " in l]
    assert naive and all(l.endswith("update=1") and f" t{l.split()[0]};" in l for l in naive)


def test_cache_files_round_trip(exe, tmp_path):
    """H2: `id|text` lines through both languages -- an empty text, unicode without '|', a rank whose file is missing; the
    fixed cache's space-separated indices, cut at --slimIPL_fixed_cache_updates; the state line resumes a run"""
    a = ipl_ref.SlimIPL("fixed-pre-cache", 1, 3, 3, 1.0, 9, 1)
    a.store(["utt-b", "utt-a", "ütt-ж", "utt-empty"], ["hello wörld", "zoo bee", "naïve 語 text", ""])
    a.save_cache(tmp_path / "in_cache0")
    c = ipl_ref.SlimIPL("fixed-pre-cache", 1, 3, 3, 1.0, 9, 1)
    c.store(["r2-x", "utt-a"], ["from rank two", "rank two wins"])      # a later rank's line replaces an earlier one (:507-509)
    c.save_cache(tmp_path / "in_cache2")
    (tmp_path / "in_fixed").write_text("4 0 8 2 6 ")
    out = subprocess.run([exe, "files", str(tmp_path), "3", "3", "9"], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out == ["rank 0: 4", "rank 1: -1", "rank 2: 2", "reused 5 rows 5", "fixed 1 3", "missing 0", "state same", "resumed same"]
    want = ipl_ref.SlimIPL("fixed-pre-cache", 1, 3, 3, 1.0, 9, 1)
    assert [want.load_cache_dump(tmp_path / f"in_cache{r}") for r in range(3)] == [4, -1, 2]
    ids = sorted(want.pl_cache_dump, key=lambda s: s.encode())
    rows, texts, reused = want.labelled(ids)
    assert reused == ids and len(rows) == 5 and want.pl_cache["utt-empty"] == "" and want.pl_cache["utt-a"] == "rank two wins"
    assert (tmp_path / "out_cache").read_bytes() == want.cache_text().encode("utf-8")
    assert "utt-empty|\n" in want.cache_text() and "ütt-ж|naïve 語 text\n" in want.cache_text()
    assert want.load_fixed_cache(tmp_path / "in_fixed") and want.fixed_cache == [4, 0, 8]
    assert (tmp_path / "out_fixed").read_text() == "4 0 8 " == want.fixed_cache_text()
    # a text never carries the line syntax into the file
    want.store(["bar"], ["a|b\nc"])
    assert "bar|a b c\n" in want.cache_text()
    # the twin's own state line resumes, too
    want.begin(); want.start_epoch()
    for _ in range(5):
        if not want.next_is_sup():
            want.next_unsup()
        want.advance_order()
    twin = ipl_ref.SlimIPL("fixed-pre-cache", 1, 3, 3, 1.0, 9, 77)
    twin.fixed_cache = list(want.fixed_cache)
    twin.set_state(want.state())
    assert twin.state() == want.state()


def test_refusals_that_need_no_device(exe):
    """H3: an unknown --slimIPL_type names the flag (the Train binary's own refusals: tests/test_gpu_train_ipl.py); the flags
    parser itself takes any --k=v line, so the new flags pass w2l_flags_check like every other"""
    out = subprocess.run([exe, "refuse", "semi-cache"], capture_output=True, text=True)
    assert out.returncode == 0 and "--slimIPL_type" in out.stdout and "semi-cache" in out.stdout
    with pytest.raises(ValueError, match="--slimIPL_type"):
        ipl_ref.SlimIPL("semi-cache", 1, 3, 2, 1.0, 3, 0)
    with pytest.raises(ValueError, match="slimIPL_sup_updates"):
        ipl_ref.SlimIPL("cache", 0, 0, 2, 1.0, 3, 0)
    from wav2letter_amd.trainer import flags_check
    assert flags_check("--slimIPL_type=cache\n--unsup_train=u.lst\n--slimIPL_ema=true\n--slimIPL_ema_decay=0.999\n") == 4


@pytest.mark.parametrize("flags,name", [
    (["--slimIPL_use_soft=true"], "--slimIPL_use_soft"),
    (["--slimIPL_type=semi-cache"], "--slimIPL_type"),
    (["--slimIPL_ema_decay=nan"], "--slimIPL_ema_decay"),
    (["--slimIPL_ema_decay=1.001"], "--slimIPL_ema_decay"),
    (["--unsup_train=u.lst", "--train=[DATA_DST]/train.lst"], "--unsup_train"),
])
def test_train_binary_refuses_before_it_touches_a_device(flags, name):
    """H3, through the binary: the slimIPL refusals come straight after the flags are read -- no arch file, no device needed"""
    exe = os.path.join(ROOT, "wav2letter_amd", "bin", "Train")
    out = subprocess.run([exe, "train", "--w2l_nlabel=30", "--arch=none.arch"] + flags, capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and out.stderr.startswith("Train: ") and name in out.stderr, (out.returncode, out.stderr)

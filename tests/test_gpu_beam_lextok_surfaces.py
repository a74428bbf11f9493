"""K9 of tests/test_gpu_beam_lextok.py: the three surfaces of the token LM under a lexicon agree -- the C ABI
(w2l_*_beam_search_lextok), Python (criterion.*_beam_search and CTCLoss / ASGLoss.beamSearch with lm_token=True), the compiled C++
beamSearch with BeamSearchOptions::lmToken (tests/cpp/decode_lextok_caller.cpp, built by tests/cpp/decode_lextok_caller.mk), the LM
and the lexicon read from the same files -- and Decode --w2l_lex_tkn=true end to end on a CTC and an ASG checkpoint (the latter
trained with --replabel=1), with the flag combinations it refuses."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ctc_beam_lm_ref as LR
from tests.list_fixture import ENV, LETTERS, UTTS
from tests.test_gpu_beam_lextok import B, FRAMES, SIL, T, classes, make_case
from tests.test_gpu_beam_sil import trained_asg  # noqa: F401  (the module-scoped ASG checkpoint, --replabel=1)
from tests.test_gpu_beam_wide import F32, KEYS, ROOT, _same_bits
from tests.test_gpu_ctc_beam import DECODE_EXE, trained  # noqa: F401  (the module-scoped CTC checkpoint)

pytestmark = pytest.mark.gpu


def test_k9_three_surfaces_agree(tmp_path):
    from tests.test_ctc_beam_lm_host import _arpa_text
    from wav2letter_amd import ASGLoss, CTCLoss, Lexicon, NGramLM, text
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "decode_lextok_caller.mk", "decode_lextok_caller", f"OUT={tmp_path}"],
                   check=True, capture_output=True)
    exe = str(tmp_path / "decode_lextok_caller")
    for i, (asg, family, score) in enumerate(((False, 0, 0.0), (False, 1, -1.5), (True, 0, -1.5), (True, 1, 0.0))):
        W = (8, 96)[family]
        c = make_case(asg, 780 + i)
        N = classes(asg)
        ntok = N if asg else N - 1
        tokens = [f"t{t}" for t in range(ntok)]
        d = tmp_path / f"case{i}"
        d.mkdir()
        (d / "tokens.txt").write_text("\n".join(tokens) + "\n")
        (d / "lex.txt").write_text("".join(f"word{w:02d} " + " ".join(tokens[t] for t in sp) + "\n" for w, sp in c.trie.rows))
        (d / "lm.arpa").write_text(_arpa_text(c.tb, tokens, unk10=-3.0)[0])
        c._lm = NGramLM.from_arpa(d / "lm.arpa", tokens)
        c._lex = Lexicon.from_file(d / "lex.txt", text.Dictionary(tokens), smearing="none", sil=tokens[SIL])
        assert c._lex.sil == SIL and c._lm.num_tokens == ntok
        c = c.but(sil=SIL if score else -1, score=score)
        M, Lmax, maxw, thr = 4, 6, 3, 8.0
        want = c.abi(family, W, 4, M, Lmax, thr, False, False, maxw)
        assert (want["lengths"] >= 0).any() and (want["word_counts"] > 0).any()
        _same_bits(c.gpu(W, 4, M, Lmax, bool(family), thr, False, False, maxw), want)
        xd, fd = torch.tensor(c.x, device="cuda"), torch.tensor(np.array(FRAMES, np.int32), device="cuda")
        opts = dict(beam=W, beam_token=4, threshold=thr, nbest=M, max_len=Lmax, wide=bool(family), lm=c._lm, lm_weight=c.lmw, eos_score=c.eos,
                    lexicon=c._lex, word_score=c.wsc, max_words=maxw, lm_token=True, sil_score=score)
        if asg:
            crit = ASGLoss(N).cuda()
            with torch.no_grad():
                crit.transitions.copy_(torch.tensor(c.A))
        else:
            crit = CTCLoss()
        got = crit.beamSearch(xd, fd, normalize=False, **opts)
        assert len(got) == len(KEYS) and all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, KEYS))
        with pytest.raises(Exception, match="xl"):
            crit.beamSearch(xd, fd, normalize=False, **dict(opts, wide="xl"))
        inp, outp = str(d / "in.bin"), str(d / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, 4, M, Lmax, maxw, 0, 0, int(asg), family, -1], np.int32).tobytes()
                    + np.array([thr, c.lmw, c.wsc, c.eos, score], F32).tobytes() + c.x.tobytes() + np.array(FRAMES, np.int32).tobytes()
                    + (c.A.tobytes() if asg else b""))
        run = subprocess.run([exe, inp, outp, str(d / "tokens.txt"), str(d / "lm.arpa"), str(d / "lex.txt"), tokens[SIL], "0"],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode lextok caller ok" in run.stdout, (i, run.returncode, run.stdout, run.stderr)
        out = np.fromfile(outp, np.int32)
        at = 0
        for k in KEYS:
            n = want[k].size
            assert (out[at:at + n] == want[k].view(np.int32).ravel()).all(), (i, k)
            at += n
        assert at == len(out)


# ---- Decode --w2l_lex_tkn=true end to end, on the six-WAV fixture of tests/list_fixture.py ---------------------------------------

def _files(tmp_path, tokens):
    from tests.test_ctc_beam_lm_host import _arpa_text
    from tests.test_gpu_ctc_beam_lex import LEX_WORDS
    (tmp_path / "lex.txt").write_text("".join(f"{w}\t{' '.join(sp)} |\n" for w, sp in LEX_WORDS))
    tb = LR.random_lm(np.random.default_rng(3), len(tokens), 3, 80)
    (tmp_path / "tokens.arpa").write_text(_arpa_text(tb, tokens, unk10=-3.0)[0])
    return tmp_path / "lex.txt", tmp_path / "tokens.arpa"


def _decode_equals_python(d, model, tmp_path, criterion):
    from wav2letter_amd import Lexicon, NGramLM, checkpoint, text
    from wav2letter_amd import criterion as crit
    from wav2letter_amd.trainer import Trainer
    asg = criterion == "asg"
    dic = text.create_token_dict(LETTERS, criterion, 1) if asg else text.create_token_dict(LETTERS, criterion)
    N = dic.index_size()
    ntok = N if asg else N - 1
    tokens = [dic.get_entry(c) for c in range(ntok)]
    lex_path, arpa = _files(tmp_path, tokens)
    lmw, wsc, eos, sil_score = 0.5, 6.0, -0.5, -1.0
    base = [DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}", "--beamsize=100", "--beamthreshold=100",
            "--uselexicon=true", "--decodertype=tkn", f"--lexicon={lex_path}", f"--lm={arpa}", f"--lmweight={lmw}", f"--wordscore={wsc}",
            f"--eosscore={eos}", "--smearing=max", "--w2l_silscore=true", f"--silscore={sil_score}", "--isbeamdump=true", "--nbest=3"]
    res = subprocess.run(base, capture_output=True, text=True, timeout=600, env=ENV)       # without the flag: the pinned refusal
    assert res.returncode != 0 and "--decodertype=tkn with --uselexicon=true: no token LM under a lexicon in this build (--decodertype=wrd)" in res.stderr
    res = subprocess.run(base + ["--w2l_lex_tkn=true", f"--w2l_dump_features={d / 'tfeat'}"], capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "--lm over the tokens" in res.stderr and "--smearing=max has no effect" in res.stderr and "(wide)" in res.stderr
    rows = [line.split(" | ") for line in (d / "out" / "other.hyp").read_text().splitlines()]
    assert rows and all(len(r) == 6 for r in rows) and any(r[5].split() for r in rows)
    for r in rows:
        score, am, lms = float(r[1]), float(r[2]), float(r[3])
        assert abs(score - (am + lmw * lms + wsc * len(r[5].split()) + eos)) <= 1e-4 * max(1.0, abs(score))

    lm = NGramLM.from_arpa(arpa, tokens)
    lex = Lexicon.from_file(lex_path, dic if asg else tokens, smearing="none", sil="|", **({"replabel": 1} if asg else {}))
    sil = dic.get_index("|")
    arch = (d / "arch" / "net.arch").read_text()
    want = []
    for k in range(3):                                                  # batches of 2, 2, 1 in list order
        utts = UTTS[2 * k:2 * k + 2][:5 - 2 * k]
        raw = (d / f"tfeat.{k + 1}").read_bytes()
        Bk, nfeat, Tk = (int(v) for v in np.frombuffer(raw[:12], np.int32))
        x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(Bk, nfeat, Tk).copy()).cuda()
        tr_ = Trainer(arch, nfeat, N, criterion, 4, 0.5 if asg else 0.0)
        checkpoint.load(str(model), tr_, arch)
        tr_.plan(Bk, Tk, 8)
        tr_.to_device()
        em = tr_.forward(x, train=False).clone()
        Tout = em.shape[1]
        frames = torch.tensor([min(max(-(-min(1 + (n - 400) // 160, Tk) * Tout // Tk), 1), Tout) for n, _ in utts], dtype=torch.int32, device="cuda")
        kw = dict(beam=100, beam_token=64, threshold=100.0, log_add=False, normalize=False, nbest=3, lm=lm, lm_weight=lmw, lexicon=lex,
                  word_score=wsc, eos_score=eos, lm_token=True, wide=True, sil_token=sil, sil_score=sil_score)
        if asg:
            A = tr_.params[tr_.n_net:tr_.n_net + N * N].view(N, N).clone()
            out = crit.asg_beam_search(em, A, frames, **kw)
        else:
            out = crit.ctc_beam_search(em, frames, **kw)
        _, _, sc, lms, wd, wc = (t.cpu().numpy() for t in out)
        for b in range(Bk):
            for m in range(3):
                if wc[b, m] >= 0:
                    want.append((f"u{2 * k + b}", f"{float(sc[b, m]):.6f}", f"{float(lms[b, m]):.6f}",
                                 " ".join(text.word_ids_to_words(wd[b, m], lex.words))))
    assert [(r[0], r[1], r[3], r[5].strip()) for r in rows] == want
    # refused by name
    for extra, name in ((["--w2l_lex_tkn=true", "--w2l_beam_xl=true"], "--w2l_beam_xl=true"), (["--w2l_lex_tkn=true", "--smearing=logadd"], "--smearing=logadd"),
                        (["--w2l_lex_tkn=true", "--unkscore=-5"], "--unkscore")):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=120, env=ENV)
        assert res.returncode != 0 and name in res.stderr, (extra, res.returncode, res.stderr[-500:])


def test_k9_decode_tool_ctc_checkpoint(trained, tmp_path):
    d, model = trained
    _decode_equals_python(d, model, tmp_path, "ctc")


def test_k9_decode_tool_asg_checkpoint_with_replabel(trained_asg, tmp_path):
    d, model = trained_asg
    _decode_equals_python(d, model, tmp_path, "asg")

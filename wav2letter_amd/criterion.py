"""Host-side mirror of fl::pkg::speech sequence criteria over the C ABI.

Mirrors (same names, argument meaning, error behaviour) the interface the
reference's Trainer uses (recipes/slimIPL/src/Train.cpp:406-410, :1675, :838;
shape of SequenceCriterion in recipes/joint_training_vox_populi/cpc/CPCCriterion.h:30-50):

  ASGLoss(N, scalemode, transdiag).forward(emission, target) -> loss[B]
  CTCLoss(scalemode).forward(emission, target) -> loss[B]
  CPCCriterion(...).get_mask(enc, mask_prob, mask_length) -> masked enc;  .forward(enc, context) -> loss[B]   (CPCCriterion.cpp:85-223)
  crit.viterbiPath(emission) -> int32 [B][T];  crit.viterbiPathWithTarget(...)

Tensors are torch CUDA(HIP) tensors used only as device buffers: emission is
[B][T][N] float32 contiguous (== ArrayFire dims (N,T,B)), target [B][L] int32
padded with -1.  Every op runs in libw2l_hip.so; there is no PyTorch fallback.
"""
import ctypes
import enum

import torch

from . import _lib


class CriterionScaleMode(enum.IntEnum):
    NONE = 0
    INPUT_SZ = 1
    INPUT_SZ_SQRT = 2
    TARGET_SZ = 3
    TARGET_SZ_SQRT = 4


def getCriterionScaleMode(onorm: str, sqnorm: bool) -> CriterionScaleMode:
    """recipes/slimIPL/src/Train.cpp:389 (--onorm / --sqnorm)"""
    if onorm == "none":
        return CriterionScaleMode.NONE
    if onorm == "input":
        return CriterionScaleMode.INPUT_SZ_SQRT if sqnorm else CriterionScaleMode.INPUT_SZ
    if onorm == "target":
        return CriterionScaleMode.TARGET_SZ_SQRT if sqnorm else CriterionScaleMode.TARGET_SZ
    raise _lib.W2LInvalidArgument(f"invalid onorm option: {onorm}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_dev(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.W2LError("w2l criteria run on the GPU only (no CPU fallback)")


def _emission_checks(emission, target=None):
    if emission.dim() != 3:
        raise _lib.W2LInvalidArgument("emission must be [B][T][N]")
    if emission.dtype != torch.float32:
        raise _lib.W2LInvalidArgument("emission must be float32")
    if target is not None:
        if target.dtype != torch.int32:
            raise _lib.W2LInvalidArgument("target must be int32")
        if target.dim() != 2 or target.shape[0] != emission.shape[0]:
            raise _lib.W2LInvalidArgument("target must be [B][L]")


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def batch_target_size(target, max_size, ctc=False):
    B, L = target.shape
    out = torch.empty(B, dtype=torch.int32, device=target.device)
    fn = _lib.lib().w2l_batch_ctc_target_size if ctc else _lib.lib().w2l_batch_target_size
    _lib.check(fn(B, L, int(max_size), target.data_ptr(), out.data_ptr(), _stream()), "batch_target_size")
    return out


class _FCC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emission, trans, target_size, scale_mode):
        L = _lib.lib()
        emission = emission.contiguous()
        trans = trans.contiguous()
        B, T, N = emission.shape
        ws = _ws(L.w2l_fcc_workspace_size(B, T, N), emission.device)
        loss = torch.empty(B, dtype=torch.float32, device=emission.device)
        _lib.check(L.w2l_fcc_forward(B, T, N, int(scale_mode), emission.data_ptr(), target_size.data_ptr(),
                                     trans.data_ptr(), loss.data_ptr(), ws.data_ptr(), _stream()), "fcc_forward")
        ctx.save_for_backward(trans, ws)
        ctx.dims = (B, T, N)
        _FCC.last = (ws, (B, T, N))   # for range_flags(): which utterances took the log-domain path (diagnostics)
        return loss

    @staticmethod
    def backward(ctx, grad):
        L = _lib.lib()
        trans, ws = ctx.saved_tensors
        B, T, N = ctx.dims
        grad = grad.contiguous().float()
        dx = torch.empty(B, T, N, dtype=torch.float32, device=grad.device)
        dt = torch.empty(N, N, dtype=torch.float32, device=grad.device)
        _lib.check(L.w2l_fcc_backward(B, T, N, trans.data_ptr(), grad.data_ptr(), dx.data_ptr(), dt.data_ptr(),
                                      ws.data_ptr(), _stream()), "fcc_backward")
        return dx, dt, None, None


class _FAC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emission, trans, target, target_size, scale_mode):
        L = _lib.lib()
        emission = emission.contiguous()
        trans = trans.contiguous()
        target = target.contiguous()
        B, T, N = emission.shape
        Lt = target.shape[1]
        ws = _ws(L.w2l_fac_workspace_size(B, T, N, Lt), emission.device)
        loss = torch.empty(B, dtype=torch.float32, device=emission.device)
        _lib.check(L.w2l_fac_forward(B, T, N, Lt, int(scale_mode), emission.data_ptr(), target.data_ptr(),
                                     target_size.data_ptr(), trans.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                     _stream()), "fac_forward")
        ctx.save_for_backward(target, target_size, ws)
        ctx.dims = (B, T, N, Lt)
        _FAC.last = (ws, (B, T, N, Lt))
        return loss

    @staticmethod
    def backward(ctx, grad):
        L = _lib.lib()
        target, target_size, ws = ctx.saved_tensors
        B, T, N, Lt = ctx.dims
        grad = grad.contiguous().float()
        dx = torch.empty(B, T, N, dtype=torch.float32, device=grad.device)
        dt = torch.empty(N, N, dtype=torch.float32, device=grad.device)
        _lib.check(L.w2l_fac_backward(B, T, N, Lt, target.data_ptr(), target_size.data_ptr(), grad.data_ptr(),
                                      dx.data_ptr(), dt.data_ptr(), ws.data_ptr(), _stream()), "fac_backward")
        return dx, dt, None, None, None


class _ASG(torch.autograd.Function):
    """ASGLoss = FullConnectionCriterion - ForceAlignmentCriterion in one call each way (w2l_asg_forward / w2l_asg_backward: the two
    criteria side by side on the current stream and a library-owned side stream, the launch sequence of the C++ criterion)"""

    @staticmethod
    def forward(ctx, emission, trans, target, scale_mode):
        L = _lib.lib()
        emission = emission.contiguous()
        trans = trans.contiguous()
        target = target.contiguous()
        B, T, N = emission.shape
        Lt = target.shape[1]
        nbytes = L.w2l_asg_workspace_size(B, T, N, Lt)
        if not nbytes:
            raise _lib.W2LError("w2l_asg_workspace_size: unsupported shape")
        ws = _ws(nbytes, emission.device)
        loss = torch.empty(B, dtype=torch.float32, device=emission.device)
        _lib.check(L.w2l_asg_forward(B, T, N, Lt, int(scale_mode), emission.data_ptr(), target.data_ptr(), trans.data_ptr(),
                                     loss.data_ptr(), ws.data_ptr(), _stream()), "asg_forward")
        ctx.save_for_backward(target, trans, ws)
        ctx.dims = (B, T, N, Lt)
        return loss

    @staticmethod
    def backward(ctx, grad):
        L = _lib.lib()
        target, trans, ws = ctx.saved_tensors
        B, T, N, Lt = ctx.dims
        grad = grad.contiguous().float()
        dx = torch.empty(B, T, N, dtype=torch.float32, device=grad.device)
        dt = torch.empty(N, N, dtype=torch.float32, device=grad.device)
        _lib.check(L.w2l_asg_backward(B, T, N, Lt, target.data_ptr(), trans.data_ptr(), grad.data_ptr(), dx.data_ptr(), dt.data_ptr(),
                                      ws.data_ptr(), _stream()), "asg_backward")
        return dx, dt, None, None


def fcc_range_flags():
    """int32 [B]: 1 where an utterance of the LAST FullConnectionCriterion forward left the range of the fp32 scaled-domain scan and
    was recomputed by the log-domain kernels (w2l_fcc_range_flags); results are exact either way"""
    ws, (B, T, N) = _FCC.last
    out = torch.empty(B, dtype=torch.int32, device=ws.device)
    _lib.check(_lib.lib().w2l_fcc_range_flags(B, T, N, ws.data_ptr(), out.data_ptr(), _stream()), "fcc_range_flags")
    return out


def fac_range_flags():
    """the same for the LAST ForceAlignmentCriterion forward (w2l_fac_range_flags)"""
    ws, (B, T, N, Lt) = _FAC.last
    out = torch.empty(B, dtype=torch.int32, device=ws.device)
    _lib.check(_lib.lib().w2l_fac_range_flags(B, T, N, Lt, ws.data_ptr(), out.data_ptr(), _stream()), "fac_range_flags")
    return out


class _FACFullPath(torch.autograd.Function):
    """ForceAlignmentCriterion on a length-T target: one alignment (w2l_fac_fullpath_*)"""

    @staticmethod
    def forward(ctx, emission, trans, path, scale_mode):
        L = _lib.lib()
        emission = emission.contiguous()
        trans = trans.contiguous()
        B, T, N = emission.shape
        loss = torch.empty(B, dtype=torch.float32, device=emission.device)
        _lib.check(L.w2l_fac_fullpath_forward(B, T, N, int(scale_mode), emission.data_ptr(), path.data_ptr(),
                                              trans.data_ptr(), loss.data_ptr(), _stream()), "fac_fullpath_forward")
        ctx.save_for_backward(path)
        ctx.dims = (B, T, N, int(scale_mode))
        return loss

    @staticmethod
    def backward(ctx, grad):
        L = _lib.lib()
        (path,) = ctx.saved_tensors
        B, T, N, mode = ctx.dims
        grad = grad.contiguous().float()
        dx = torch.empty(B, T, N, dtype=torch.float32, device=grad.device)
        dt = torch.empty(N, N, dtype=torch.float32, device=grad.device)
        _lib.check(L.w2l_fac_fullpath_backward(B, T, N, mode, path.data_ptr(), grad.data_ptr(), dx.data_ptr(),
                                               dt.data_ptr(), _stream()), "fac_fullpath_backward")
        return dx, dt, None, None


def linear_target(target, T):
    """Flashlight getLinearTarget: [B][L] labels (-1 padded) stretched to [B][T]"""
    _check_dev(target)
    target = target.contiguous()
    B, L = target.shape
    out = torch.empty(B, T, dtype=torch.int32, device=target.device)
    _lib.check(_lib.lib().w2l_linear_target(B, L, int(T), target.data_ptr(), out.data_ptr(), _stream()), "linear_target")
    return out


class _CTC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emission, target, target_size, scale_mode):
        L = _lib.lib()
        emission = emission.contiguous()
        target = target.contiguous()
        B, T, N = emission.shape
        Lt = target.shape[1]
        ws = _ws(L.w2l_ctc_workspace_size(B, T, N, Lt), emission.device)
        loss = torch.empty(B, dtype=torch.float32, device=emission.device)
        _lib.check(L.w2l_ctc_forward(B, T, N, Lt, int(scale_mode), emission.data_ptr(), target.data_ptr(),
                                     target_size.data_ptr(), loss.data_ptr(), ws.data_ptr(), _stream()),
                   "ctc_forward")
        ctx.save_for_backward(emission, target, target_size, ws)
        ctx.dims = (B, T, N, Lt)
        return loss

    @staticmethod
    def backward(ctx, grad):
        L = _lib.lib()
        emission, target, target_size, ws = ctx.saved_tensors
        B, T, N, Lt = ctx.dims
        grad = grad.contiguous().float()
        dx = torch.empty(B, T, N, dtype=torch.float32, device=grad.device)
        _lib.check(L.w2l_ctc_backward(B, T, N, Lt, emission.data_ptr(), target.data_ptr(), target_size.data_ptr(),
                                      grad.data_ptr(), dx.data_ptr(), ws.data_ptr(), _stream()), "ctc_backward")
        return dx, None, None, None


def ctc_score(emission, target, scalemode=CriterionScaleMode.NONE):
    """CTC evaluation in one read of the emissions (w2l_ctc_score): returns (loss [B] float32, path [B][T] int32), bitwise equal
    to CTCLoss.forward and CTCLoss.viterbiPath.  No gradient: the loss does not take part in autograd."""
    _emission_checks(emission, target)
    _check_dev(emission, target)
    L = _lib.lib()
    emission = emission.detach().contiguous()
    target = target.contiguous()
    B, T, N = emission.shape
    Lt = target.shape[1]
    ts = batch_target_size(target, T, ctc=True)
    ws = _ws(L.w2l_ctc_score_workspace_size(B, T, N, Lt), emission.device)
    loss = torch.empty(B, dtype=torch.float32, device=emission.device)
    path = torch.empty(B, T, dtype=torch.int32, device=emission.device)
    _lib.check(L.w2l_ctc_score(B, T, N, Lt, int(scalemode), emission.data_ptr(), target.data_ptr(), ts.data_ptr(),
                               loss.data_ptr(), path.data_ptr(), ws.data_ptr(), _stream()), "ctc_score")
    return loss, path


def ctc_align(emission, target, frames=None, with_score=True):
    """CTC forced alignment (w2l_ctc_align): the most probable lattice path of the known transcript `target` [B][L] (negative =
    padding) through `emission` [B][T][N], blank = N-1.  `frames` [B] int32: the emission frames that belong to each utterance,
    1..T (None: all T); frames beyond them are filled with blank.  Returns (path [B][T] int32, score [B] float32 or None): the
    path is bit-exact with the fp32 max-plus recursion on the raw emissions (stay beats advance beats skip on ties), the score is
    its log-probability under the softmax.  A target that does not fit its frames gives a row of -1 and score -inf."""
    _emission_checks(emission, target)
    _check_dev(emission, target)
    L = _lib.lib()
    emission = emission.detach().contiguous()
    target = target.contiguous()
    B, T, N = emission.shape
    Lt = target.shape[1]
    if frames is not None:
        if frames.dtype != torch.int32 or frames.numel() != B:
            raise _lib.W2LInvalidArgument("ctc_align: frames must be int32 with one entry per utterance")
        _check_dev(emission, frames)
        frames = frames.contiguous()
    ts = batch_target_size(target, T, ctc=True)
    ws = _ws(L.w2l_ctc_align_workspace_size(B, T, N, Lt), emission.device)
    path = torch.empty(B, T, dtype=torch.int32, device=emission.device)
    score = torch.empty(B, dtype=torch.float32, device=emission.device) if with_score else None
    _lib.check(L.w2l_ctc_align(B, T, N, Lt, emission.data_ptr(), target.data_ptr(), ts.data_ptr(),
                               frames.data_ptr() if frames is not None else None, path.data_ptr(),
                               score.data_ptr() if with_score else None, ws.data_ptr(), _stream()), "ctc_align")
    return path, score


def _wide_checks(wide, lm_token):
    """what `wide` may be, alone and with lm_token, refused before anything else looks at the call"""
    if isinstance(wide, str) and wide not in ("xl", "mt"):
        raise _lib.W2LInvalidArgument(f'beam search: wide must be False, True, "xl" or "mt", not {wide!r}')
    if lm_token and wide == "mt":
        raise _lib.W2LInvalidArgument('beam search: lm_token=True has no many-token family (wide must be False or True)')


def _beam_family(wide, lm_token=False):
    """the w2l_beam_family `wide` names: False narrow, True wide, "xl", "mt"; lm_token=True has the first two only"""
    _wide_checks(wide, lm_token)
    if lm_token and wide == "xl":
        raise _lib.W2LInvalidArgument('beam search: lm_token=True has no xl family (wide must be False or True)')
    if isinstance(wide, str):
        return _lib.BEAM_XL if wide == "xl" else _lib.BEAM_MT
    return _lib.BEAM_WIDE if wide else _lib.BEAM_NARROW


def _beam_search(who, wide, lm_token, kind, sil, device, **fields):
    """one w2l_beam_search call on a workspace of its size: `fields` are w2l_beam_search_desc's, sil = (token, score) or None"""
    L = _lib.lib()
    tok, score = sil if sil is not None else (-1, 0.0)
    d = _lib.BeamSearchDesc(family=_beam_family(wide, lm_token), kind=kind, silToken=tok, silScore=score, **fields)
    ws = _ws(L.w2l_beam_search_workspace_size(ctypes.byref(d)), device)
    _lib.check(L.w2l_beam_search(ctypes.byref(d), ws.data_ptr(), _stream()), who)


def _sil_args(who, sil_token, sil_score, lexicon):
    """(token, score) for the *_sil entry points, or None: the call without a silence score.  sil_token None: the lexicon's"""
    sil_score = float(sil_score)
    if sil_token is None and lexicon is not None and lexicon.sil >= 0:
        sil_token = lexicon.sil
    if sil_token is None:
        if sil_score != 0.0:
            raise _lib.W2LInvalidArgument(f"{who}: sil_score needs a silence token (sil_token=, or a lexicon that has one)")
        return None
    if sil_score == 0.0 and int(sil_token) == -1:
        return None
    return int(sil_token), sil_score


def ctc_beam_search(emission, frames=None, beam=64, beam_token=64, threshold=float("inf"), log_add=False, normalize=None,
                    nbest=1, max_len=None, lm=None, lm_weight=0.0, class_score=None, eos_score=0.0, lexicon=None, word_score=0.0,
                    max_words=None, wide=False, sil_token=None, sil_score=0.0, lm_token=False):
    """CTC prefix beam search without lexicon or LM (w2l_ctc_beam_search; the contract is in include/w2l_hip.h): `emission`
    [B][T][N], blank = N-1, `frames` [B] int32 as in ctc_align.  beam = W (<= 64; <= 1024 with wide=True; <= 8192 with wide="xl"), beam_token = K (clipped to N-1, then <= 64; <= 256 with wide="mt"),
    log_add: sum (True) or max (False) over the alignments of a prefix; normalize: search on log-softmax rows (default: log_add --
    sums only mean something on log-probabilities; the max search runs on the raw emissions as the reference's decoder does).
    Returns (labels [B][nbest][max_len] int32, -1 beyond a hypothesis; lengths [B][nbest] int32, the true label counts, -1 for a
    rank that does not exist; scores [B][nbest] float32, -inf there).  max_len defaults to T (no hypothesis is longer).
    lm: an lm.NGramLM over the N-1 token classes: the search fused with it (w2l_ctc_beam_search_lm): every extension by token c
    adds lm_weight * log p_LM(c | prefix) + class_score[c] (class_score: [N-1] float32 on the device, or None), the end adds
    lm_weight * log p_LM(EOS | hypothesis) + eos_score when the model has EOS.  Returns a fourth tensor then: lm_scores [B][nbest],
    the hypotheses' unweighted LM scores.  Without lm the other three arguments must keep their defaults.
    lexicon: a lexicon.Lexicon over the N-1 token classes: the search restricted to its spellings (w2l_ctc_beam_search_lex).  lm is
    required then and is an NGramLM over the lexicon's WORDS (NGramLM.from_arpa(path, lexicon.words)); class_score must be None;
    every completed word adds lm_weight * log p_LM(word | words before) + word_score, smeared down the trie.  Returns
    (labels, lengths, scores, lm_scores, words [B][nbest][max_words] int32 word ids, -1 beyond; word_counts [B][nbest] int32);
    max_words defaults to max_len.  A hypothesis that ends inside a word does not count: an utterance may have only empty rows.
    wide: run the wide kernels (the w2l_*_wide entry points): the same contract with beam up to 1024; beam_token stays <= 64.  At
    beam <= 64 both kernel families return the same bytes.  wide="xl": run the xl kernels (the w2l_*_xl entry points): the same
    contract with beam up to 8192, the widths the reference's decoding recipes ask for; at beam <= 1024 they return the wide
    kernels' bytes.  No family is chosen for the caller: wide=True with beam > 1024 is refused as before.  wide="mt": run the
    many-token kernels (the w2l_*_mt entry points): beam up to 8192 as with "xl" and beam_token, after clipping, up to 256 -- the
    --beamsizetoken of the reference's word-piece recipes (100, 150); at beam_token <= 64 they return the xl kernels' bytes.
    sil_token, sil_score: the silence score (the w2l_*_sil entry points; the reference's --silscore): after the frame tokens have
    been chosen by the acoustic lp alone, class sil_token's frame score is lp + sil_score wherever the search reads it.
    sil_token=None with a lexicon: the lexicon's silence token.  A non-zero sil_score without any silence token is refused;
    sil_score = 0 is the search without a silence score, the same bytes.
    lm_token=True (needs lexicon; w2l_ctc_beam_search_lextok, the reference's --uselexicon=true --decodertype=tkn): lm is an NGramLM
    over the lexicon's TOKENS, not its words.  Every token that moves along a trie edge adds lm_weight * log p_LM(token | tokens
    before), a completed word adds word_score alone, the lexicon's smear values are not read.  The return values are the lexicon
    search's.  wide=True for beams up to 1024; wide="xl" and wide="mt" are refused."""
    _wide_checks(wide, lm_token)
    _emission_checks(emission)
    B, T, N = emission.shape
    sil = _sil_args("ctc_beam_search", sil_token, sil_score, lexicon)
    if lm_token and lexicon is None:
        raise ValueError("ctc_beam_search: lm_token=True needs lexicon (without one, lm alone is the token-LM search)")
    if lm_token and lm is not None and lm.num_tokens != lexicon.num_tokens:
        raise ValueError(f"ctc_beam_search: lm_token=True: the LM has {lm.num_tokens} tokens, the lexicon {lexicon.num_tokens}")
    if lexicon is not None:
        if lm is None:
            raise _lib.W2LInvalidArgument("ctc_beam_search: lexicon needs lm, a model over the lexicon's words")
        if class_score is not None:
            raise _lib.W2LInvalidArgument("ctc_beam_search: class_score must be None with a lexicon (word_score is the per-word term)")
        if not lm_token and lm.num_tokens != lexicon.num_words:
            raise _lib.W2LInvalidArgument(f"ctc_beam_search: the LM has {lm.num_tokens} words, the lexicon {lexicon.num_words}")
        if lexicon.num_tokens != N - 1:
            raise _lib.W2LInvalidArgument(f"ctc_beam_search: the lexicon has {lexicon.num_tokens} tokens, the emissions {N - 1}")
        if not lm.has_eos and eos_score != 0.0:
            raise _lib.W2LInvalidArgument("ctc_beam_search: eos_score needs a model with EOS")
        if max_words is not None and int(max_words) < 1:
            raise _lib.W2LInvalidArgument("ctc_beam_search: max_words must be at least 1")
    elif word_score != 0.0 or max_words is not None:
        raise _lib.W2LInvalidArgument("ctc_beam_search: word_score and max_words need lexicon")
    elif lm is None:
        if lm_weight != 0.0 or class_score is not None or eos_score != 0.0:
            raise _lib.W2LInvalidArgument("ctc_beam_search: lm_weight, class_score and eos_score need lm")
    else:
        if lm.num_tokens != N - 1:
            raise _lib.W2LInvalidArgument(f"ctc_beam_search: the LM has {lm.num_tokens} tokens, the emissions {N - 1}")
        if not lm.has_eos and eos_score != 0.0:
            raise _lib.W2LInvalidArgument("ctc_beam_search: eos_score needs a model with EOS")
        if class_score is not None and (class_score.dtype != torch.float32 or class_score.numel() != N - 1):
            raise _lib.W2LInvalidArgument("ctc_beam_search: class_score must be float32 with one entry per token class")
    _check_dev(emission)
    _lib.lib()
    emission = emission.detach().contiguous()
    if frames is not None:
        if frames.dtype != torch.int32 or frames.numel() != B:
            raise _lib.W2LInvalidArgument("ctc_beam_search: frames must be int32 with one entry per utterance")
        _check_dev(emission, frames)
        frames = frames.contiguous()
    if normalize is None:
        normalize = bool(log_add)
    max_len = T if max_len is None else int(max_len)
    nbest = int(nbest)
    shape = (B, max(nbest, 1))
    labels = torch.empty(*shape, max(max_len, 1), dtype=torch.int32, device=emission.device)
    lengths = torch.empty(*shape, dtype=torch.int32, device=emission.device)
    scores = torch.empty(*shape, dtype=torch.float32, device=emission.device)
    common = dict(B=B, T=T, N=N, input=emission.data_ptr(), frames=frames.data_ptr() if frames is not None else None, beam=int(beam),
                  beamToken=int(beam_token), threshold=float(threshold), logAdd=int(bool(log_add)), normalize=int(bool(normalize)),
                  nbest=nbest, maxLen=max_len, labels=labels.data_ptr(), lengths=lengths.data_ptr(), scores=scores.data_ptr())
    if lm is None:
        _beam_search("ctc_beam_search", wide, lm_token, _lib.SEARCH_PLAIN, sil, emission.device, **common)
        return labels, lengths, scores
    lm_scores = torch.empty(*shape, dtype=torch.float32, device=emission.device)
    blob = lm.device_blob(emission.device)
    common.update(lm=blob.data_ptr(), lmHasEos=int(lm.has_eos), lmWeight=float(lm_weight), eosScore=float(eos_score),
                  lmScores=lm_scores.data_ptr())
    if lexicon is not None:
        max_words = max(max_len, 1) if max_words is None else int(max_words)
        words = torch.empty(*shape, max_words, dtype=torch.int32, device=emission.device)
        word_counts = torch.empty(*shape, dtype=torch.int32, device=emission.device)
        lex_blob = lexicon.device_blob(emission.device)
        _beam_search("ctc_beam_search", wide, lm_token, _lib.SEARCH_LEXTOK if lm_token else _lib.SEARCH_LEX, sil, emission.device,
                     lexicon=lex_blob.data_ptr(), wordScore=float(word_score), maxWords=max_words, words=words.data_ptr(),
                     wordCounts=word_counts.data_ptr(), **common)
        return labels, lengths, scores, lm_scores, words, word_counts
    if class_score is not None:
        _check_dev(emission, class_score)
        class_score = class_score.contiguous()
    _beam_search("ctc_beam_search", wide, lm_token, _lib.SEARCH_LM, sil, emission.device,
                 classScore=class_score.data_ptr() if class_score is not None else None, **common)
    return labels, lengths, scores, lm_scores


def asg_beam_search(emission, transitions, frames=None, beam=64, beam_token=64, threshold=float("inf"), log_add=False, normalize=False,
                    nbest=1, max_len=None, lm=None, lm_weight=0.0, class_score=None, eos_score=0.0, lexicon=None, word_score=0.0,
                    max_words=None, wide=False, sil_token=None, sil_score=0.0, lm_token=False):
    """Beam search of an ASG model (w2l_asg_beam_search, w2l_asg_beam_search_lex; the contract is in include/w2l_hip.h):
    `emission` [B][T][N], every class a token (no blank), `transitions` [N][N] float32 (to x from) on the emissions' device.  The
    options and the return values are ctc_beam_search's -- (labels, lengths, scores), lm_scores with an LM, words and word_counts
    with a lexicon -- with beam_token clipped to N, an LM (or lexicon) over N tokens and class_score [N].  normalize defaults to
    False in both log_add modes: ASG scores are unnormalised by design.  A token never follows itself: a repeated letter is a
    replabel's (Lexicon.from_file(..., replabel=) packs the spellings).  wide, sil_token, sil_score, lm_token: as in ctc_beam_search."""
    _wide_checks(wide, lm_token)
    _emission_checks(emission)
    B, T, N = emission.shape
    sil = _sil_args("asg_beam_search", sil_token, sil_score, lexicon)
    if lm_token and lexicon is None:
        raise ValueError("asg_beam_search: lm_token=True needs lexicon (without one, lm alone is the token-LM search)")
    if lm_token and lm is not None and lm.num_tokens != lexicon.num_tokens:
        raise ValueError(f"asg_beam_search: lm_token=True: the LM has {lm.num_tokens} tokens, the lexicon {lexicon.num_tokens}")
    if transitions.dtype != torch.float32 or tuple(transitions.shape) != (N, N):
        raise _lib.W2LInvalidArgument(f"asg_beam_search: transitions must be float32 [{N}][{N}]")
    if lexicon is not None:
        if lm is None:
            raise _lib.W2LInvalidArgument("asg_beam_search: lexicon needs lm, a model over the lexicon's words")
        if class_score is not None:
            raise _lib.W2LInvalidArgument("asg_beam_search: class_score must be None with a lexicon (word_score is the per-word term)")
        if not lm_token and lm.num_tokens != lexicon.num_words:
            raise _lib.W2LInvalidArgument(f"asg_beam_search: the LM has {lm.num_tokens} words, the lexicon {lexicon.num_words}")
        if lexicon.num_tokens != N:
            raise _lib.W2LInvalidArgument(f"asg_beam_search: the lexicon has {lexicon.num_tokens} tokens, the emissions {N}")
        if max_words is not None and int(max_words) < 1:
            raise _lib.W2LInvalidArgument("asg_beam_search: max_words must be at least 1")
    elif word_score != 0.0 or max_words is not None:
        raise _lib.W2LInvalidArgument("asg_beam_search: word_score and max_words need lexicon")
    elif lm is None:
        if lm_weight != 0.0 or class_score is not None or eos_score != 0.0:
            raise _lib.W2LInvalidArgument("asg_beam_search: lm_weight, class_score and eos_score need lm")
    else:
        if lm.num_tokens != N:
            raise _lib.W2LInvalidArgument(f"asg_beam_search: the LM has {lm.num_tokens} tokens, the emissions {N}")
        if class_score is not None and (class_score.dtype != torch.float32 or class_score.numel() != N):
            raise _lib.W2LInvalidArgument("asg_beam_search: class_score must be float32 with one entry per class")
    if lm is not None and not lm.has_eos and eos_score != 0.0:
        raise _lib.W2LInvalidArgument("asg_beam_search: eos_score needs a model with EOS")
    _check_dev(emission, transitions)
    _lib.lib()
    emission = emission.detach().contiguous()
    transitions = transitions.detach().contiguous()
    if frames is not None:
        if frames.dtype != torch.int32 or frames.numel() != B:
            raise _lib.W2LInvalidArgument("asg_beam_search: frames must be int32 with one entry per utterance")
        _check_dev(emission, frames)
        frames = frames.contiguous()
    fr = frames.data_ptr() if frames is not None else None
    max_len = T if max_len is None else int(max_len)
    nbest = int(nbest)
    shape = (B, max(nbest, 1))
    dev = emission.device
    labels = torch.empty(*shape, max(max_len, 1), dtype=torch.int32, device=dev)
    lengths = torch.empty(*shape, dtype=torch.int32, device=dev)
    scores = torch.empty(*shape, dtype=torch.float32, device=dev)
    lm_scores = torch.empty(*shape, dtype=torch.float32, device=dev)
    common = dict(B=B, T=T, N=N, input=emission.data_ptr(), frames=fr, trans=transitions.data_ptr(), beam=int(beam),
                  beamToken=int(beam_token), threshold=float(threshold), logAdd=int(bool(log_add)), normalize=int(bool(normalize)),
                  nbest=nbest, maxLen=max_len, labels=labels.data_ptr(), lengths=lengths.data_ptr(), scores=scores.data_ptr(),
                  lmScores=lm_scores.data_ptr(), lmWeight=float(lm_weight), eosScore=float(eos_score))
    if lm is not None:
        blob = lm.device_blob(dev)
        common.update(lm=blob.data_ptr(), lmHasEos=int(lm.has_eos))
    if lexicon is not None:
        max_words = max(max_len, 1) if max_words is None else int(max_words)
        words = torch.empty(*shape, max_words, dtype=torch.int32, device=dev)
        word_counts = torch.empty(*shape, dtype=torch.int32, device=dev)
        lex_blob = lexicon.device_blob(dev)
        _beam_search("asg_beam_search", wide, lm_token, _lib.SEARCH_LEXTOK if lm_token else _lib.SEARCH_LEX, sil, dev,
                     lexicon=lex_blob.data_ptr(), wordScore=float(word_score), maxWords=max_words, words=words.data_ptr(),
                     wordCounts=word_counts.data_ptr(), **common)
        return labels, lengths, scores, lm_scores, words, word_counts
    if class_score is not None:
        _check_dev(emission, class_score)
        class_score = class_score.contiguous()
    _beam_search("asg_beam_search", wide, lm_token, _lib.SEARCH_LM if lm is not None else _lib.SEARCH_PLAIN, sil, dev,
                 classScore=class_score.data_ptr() if class_score is not None else None, **common)
    return (labels, lengths, scores, lm_scores) if lm is not None else (labels, lengths, scores)


class SequenceCriterion(torch.nn.Module):
    """fl::pkg::speech::SequenceCriterion: forward({emission,target}) -> {loss[B]},
    viterbiPath(emission) -> [B][T] int32."""

    def prettyString(self):
        return type(self).__name__


class FullConnectionCriterion(SequenceCriterion):
    def __init__(self, N, scalemode=CriterionScaleMode.NONE, transitions=None):
        super().__init__()
        self.N, self.scalemode = N, scalemode
        self.transitions = transitions if transitions is not None else torch.nn.Parameter(torch.zeros(N, N))

    def forward(self, emission, target):
        _emission_checks(emission, target)
        _check_dev(emission, target)
        if emission.shape[2] != self.N:
            raise _lib.W2LInvalidArgument("FullConnectionCriterion: N doesn't match with the letter size")
        ts = batch_target_size(target, emission.shape[1])
        return _FCC.apply(emission, self.transitions, ts, self.scalemode)


class ForceAlignmentCriterion(SequenceCriterion):
    def __init__(self, N, scalemode=CriterionScaleMode.NONE, transitions=None):
        super().__init__()
        self.N, self.scalemode = N, scalemode
        self.transitions = transitions if transitions is not None else torch.nn.Parameter(torch.zeros(N, N))

    def forward(self, emission, target):
        _emission_checks(emission, target)
        _check_dev(emission, target)
        if emission.shape[2] != self.N:
            raise _lib.W2LInvalidArgument("ForceAlignmentCriterion: N doesn't match with the letter size")
        ts = batch_target_size(target, emission.shape[1])
        return _FAC.apply(emission, self.transitions, target, ts, self.scalemode)

    def viterbiPath(self, emission, target):
        _emission_checks(emission, target)
        L = _lib.lib()
        emission = emission.contiguous()
        B, T, N = emission.shape
        Lt = target.shape[1]
        ts = batch_target_size(target, T)
        ws = _ws(L.w2l_fac_workspace_size(B, T, N, Lt), emission.device)
        path = torch.empty(B, T, dtype=torch.int32, device=emission.device)
        _lib.check(L.w2l_fac_viterbi(B, T, N, Lt, emission.data_ptr(), target.data_ptr(), ts.data_ptr(),
                                     self.transitions.detach().contiguous().data_ptr(), path.data_ptr(),
                                     ws.data_ptr(), _stream()), "fac_viterbi")
        return path


class ASGLoss(SequenceCriterion):
    """AutoSegmentationCriterion = FCC - FAC sharing one N x N transition
    parameter initialised to transdiag * I (recipes/slimIPL/src/Train.cpp:410;
    --transdiag, recipes/conv_glu/librispeech/train.cfg:25)."""

    def __init__(self, N, scalemode=CriterionScaleMode.NONE, transdiag=0.0):
        super().__init__()
        self.N, self.scalemode = N, scalemode
        self.transitions = torch.nn.Parameter(torch.eye(N) * float(transdiag))
        self.fac = ForceAlignmentCriterion(N, scalemode, self.transitions)
        self.fcc = FullConnectionCriterion(N, scalemode, self.transitions)
        self._side = None

    def forward(self, emission, target):
        # FCC and FAC are independent length-T serial scans that use B of the 256 CUs each: w2l_asg_forward / w2l_asg_backward run
        # them side by side (one call each way: the C++ criterion's launch sequence, fused for the letter-sized label sets)
        if not emission.is_cuda:
            return self.fcc(emission, target) - self.fac(emission, target)  # raises the reference's error
        _emission_checks(emission, target)
        _check_dev(emission, target)
        if emission.shape[2] != self.N:
            raise _lib.W2LInvalidArgument("ASGLoss: N doesn't match with the letter size")
        return _ASG.apply(emission, self.transitions, target, self.scalemode)

    def viterbiPath(self, emission, inputSize=None):
        _emission_checks(emission)
        _check_dev(emission)
        L = _lib.lib()
        emission = emission.contiguous()
        B, T, N = emission.shape
        ws = _ws(L.w2l_viterbi_workspace_size(B, T, N), emission.device)
        path = torch.empty(B, T, dtype=torch.int32, device=emission.device)
        _lib.check(L.w2l_viterbi_compute(B, T, N, emission.data_ptr(),
                                         self.transitions.detach().contiguous().data_ptr(), path.data_ptr(),
                                         ws.data_ptr(), _stream()), "viterbi_compute")
        return path

    def viterbiPathWithTarget(self, emission, target):
        return self.fac.viterbiPath(emission, target)

    def beamSearch(self, emission, frames=None, **options):
        """n-best beam search over the emissions under this criterion's transitions (asg_beam_search's options; wide=True: beam
        up to 1024, wide="xl": up to 8192, wide="mt": up to 8192 with beam_token up to 256)"""
        return asg_beam_search(emission, self.transitions, frames, **options)

    def prettyString(self):
        return "AutoSegmentationCriterion"


class LinSegCriterion(SequenceCriterion):
    """LinearSegmentationCriterion: ASG on the target stretched linearly over the T frames, used for the first
    --linseg updates of every ASG recipe with the ASG criterion's own transition parameter
    (`linseg->setParams(criterion->param(0), 0)`, recipes/slimIPL/src/Train.cpp:592-596)."""

    def __init__(self, N, scalemode=CriterionScaleMode.NONE, transitions=None):
        super().__init__()
        self.N, self.scalemode = N, scalemode
        self.transitions = transitions if transitions is not None else torch.nn.Parameter(torch.zeros(N, N))

    def setParams(self, var, pos=0):
        if pos != 0:
            raise _lib.W2LInvalidArgument("LinSegCriterion has one parameter (transitions)")
        self.transitions = var

    def forward(self, emission, target):
        _emission_checks(emission, target)
        _check_dev(emission, target)
        if emission.shape[2] != self.N:
            raise _lib.W2LInvalidArgument("LinSegCriterion: N doesn't match with the letter size")
        T = emission.shape[1]
        lin = linear_target(target, T)
        ts = batch_target_size(lin, T)          # T, or 0 for a row that could not be stretched
        fcc = _FCC.apply(emission, self.transitions, ts, self.scalemode)
        fac = _FACFullPath.apply(emission, self.transitions, lin, self.scalemode)
        return fcc - fac

    def prettyString(self):
        return "LinearSegmentationCriterion"


class CTCLoss(SequenceCriterion):
    """ConnectionistTemporalClassificationCriterion(scalemode); blank = N-1"""

    def __init__(self, scalemode=CriterionScaleMode.NONE):
        super().__init__()
        self.scalemode = scalemode

    def forward(self, emission, target):
        _emission_checks(emission, target)
        _check_dev(emission, target)
        ts = batch_target_size(target, emission.shape[1], ctc=True)
        return _CTC.apply(emission, target, ts, self.scalemode)

    def viterbiPath(self, emission, inputSize=None):
        _emission_checks(emission)
        _check_dev(emission)
        emission = emission.contiguous()
        B, T, N = emission.shape
        path = torch.empty(B, T, dtype=torch.int32, device=emission.device)
        _lib.check(_lib.lib().w2l_ctc_viterbi(B, T, N, emission.data_ptr(), path.data_ptr(), _stream()),
                   "ctc_viterbi")
        return path

    def viterbiPathWithTarget(self, emission, target, frames=None):
        """forced alignment of `target` to the emissions: [B][T] int32, one label per frame (ctc_align without the score)"""
        return ctc_align(emission, target, frames, with_score=False)[0]

    def beamSearch(self, emission, frames=None, **options):
        """n-best beam search over the emissions (ctc_beam_search's options, lm= and lexicon= included): (labels, lengths, scores),
        lm_scores with an LM, and words and word_counts with a lexicon.  wide=True: beam up to 1024, wide="xl": up to 8192,
        wide="mt": up to 8192 with beam_token up to 256"""
        return ctc_beam_search(emission, frames, **options)

    def score(self, emission, target):
        """(loss [B], viterbiPath [B][T]) of a held-out batch in one pass over the emissions (ctc_score)"""
        return ctc_score(emission, target, self.scalemode)

    def prettyString(self):
        return "ConnectionistTemporalClassificationCriterion"


class _CPCMask(torch.autograd.Function):
    """y = mask ? emb : x over [B][T][C] (w2l_cpc_apply_mask / w2l_cpc_apply_mask_backward); mask: uint8 [B][T] on the device"""

    @staticmethod
    def forward(ctx, x, emb, mask):
        L = _lib.lib()
        x = x.contiguous()
        emb = emb.contiguous()
        B, T, C = x.shape
        y = torch.empty_like(x)
        _lib.check(L.w2l_cpc_apply_mask(B, T, C, x.data_ptr(), mask.data_ptr(), emb.data_ptr(), y.data_ptr(), _stream()), "cpc_apply_mask")
        ctx.save_for_backward(mask)
        ctx.dims = (B, T, C)
        return y

    @staticmethod
    def backward(ctx, grad):
        L = _lib.lib()
        (mask,) = ctx.saved_tensors
        B, T, C = ctx.dims
        grad = grad.contiguous().float()
        dx = torch.empty_like(grad)
        demb = torch.empty(C, dtype=torch.float32, device=grad.device)
        ws = _ws(L.w2l_cpc_mask_workspace_size(B, T, C), grad.device)
        _lib.check(L.w2l_cpc_apply_mask_backward(B, T, C, grad.data_ptr(), mask.data_ptr(), dx.data_ptr(), demb.data_ptr(), ws.data_ptr(),
                                                 _stream()), "cpc_apply_mask_backward")
        return dx, demb, None


class _CPC(torch.autograd.Function):
    """the InfoNCE loss of the masked frames (w2l_cpc_forward / w2l_cpc_backward; the contract is in include/w2l_hip.h)"""

    @staticmethod
    def forward(ctx, enc, context, We, be, Wc, bc, mask_index, neg, tau):
        L = _lib.lib()
        enc, context = enc.contiguous(), context.contiguous()
        We, be, Wc, bc = We.contiguous(), be.contiguous(), Wc.contiguous(), bc.contiguous()
        B, T, Ce = enc.shape
        Cc, D = context.shape[2], We.shape[0]
        M, K = mask_index.shape[1], neg.shape[2]
        nbytes = L.w2l_cpc_workspace_size(B, T, Ce, Cc, D, M, K)
        if not nbytes:
            raise _lib.W2LInvalidArgument(f"w2l_cpc_workspace_size: shape B={B} T={T} Ce={Ce} Cc={Cc} D={D} M={M} K={K} is refused")
        ws = _ws(nbytes, enc.device)
        loss = torch.empty(B, dtype=torch.float32, device=enc.device)
        _lib.check(L.w2l_cpc_forward(B, T, Ce, Cc, D, M, K, float(tau), enc.data_ptr(), context.data_ptr(), mask_index.data_ptr(),
                                     neg.data_ptr(), We.data_ptr(), be.data_ptr(), Wc.data_ptr(), bc.data_ptr(), loss.data_ptr(),
                                     ws.data_ptr(), _stream()), "cpc_forward")
        ctx.save_for_backward(We, Wc, mask_index, neg, ws)
        ctx.dims = (B, T, Ce, Cc, D, M, K, float(tau))
        return loss

    @staticmethod
    def backward(ctx, grad):
        L = _lib.lib()
        We, Wc, mask_index, neg, ws = ctx.saved_tensors
        B, T, Ce, Cc, D, M, K, tau = ctx.dims
        grad = grad.contiguous().float()
        dev = grad.device
        denc = torch.empty(B, T, Ce, dtype=torch.float32, device=dev)
        dctx = torch.empty(B, T, Cc, dtype=torch.float32, device=dev)
        dWe, dbe = torch.empty(D, Ce, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        dWc, dbc = torch.empty(D, Cc, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        _lib.check(L.w2l_cpc_backward(B, T, Ce, Cc, D, M, K, tau, mask_index.data_ptr(), neg.data_ptr(), We.data_ptr(), Wc.data_ptr(),
                                      grad.data_ptr(), denc.data_ptr(), dctx.data_ptr(), dWe.data_ptr(), dbe.data_ptr(), dWc.data_ptr(),
                                      dbc.data_ptr(), ws.data_ptr(), _stream()), "cpc_backward")
        return denc, dctx, dWe, dbe, dWc, dbc, None, None, None


class CPCCriterion(SequenceCriterion):
    """The criterion of the reference's self-supervised trainer (--criterion=cpc, recipes/joint_training_vox_populi/cpc/
    CPCCriterion.cpp): get_mask replaces spans of the encoder output by a learned embedding before the context network sees it,
    forward scores every masked frame's context against its own encoder output and K negatives, other masked frames of the same
    utterance.  Parameters in the reference's order: the mask embedding [nEncoder], uniform in (-1, 1); the encoder projection's
    weight [nMutual][nEncoder] and bias; the context projection's weight [nMutual][nContext] and bias (fl::Linear's initialisation:
    uniform within 1 / sqrt(fan-in)).  nOffset, nUnits, nPieces and nBuffer are stored and unused, exactly as in the reference.
    The draws are this project's seeded stream (wav2letter_amd/cpc.py), not ArrayFire's."""

    def __init__(self, nEncoder, nContext, nMutual, nOffset, nUnits, nPieces, nNegative, nBuffer, temperature):
        super().__init__()
        self.nEncoder, self.nContext, self.nMutual = int(nEncoder), int(nContext), int(nMutual)
        self.nOffset, self.nUnits, self.nPieces, self.nBuffer = nOffset, nUnits, nPieces, nBuffer
        self.nNegative, self.temperature = int(nNegative), float(temperature)
        self.mask_embedding = torch.nn.Parameter(torch.empty(self.nEncoder).uniform_(-1.0, 1.0))
        for name, fan_in in (("encoder", self.nEncoder), ("context", self.nContext)):
            bound = fan_in ** -0.5
            setattr(self, name + "_weight", torch.nn.Parameter(torch.empty(self.nMutual, fan_in).uniform_(-bound, bound)))
            setattr(self, name + "_bias", torch.nn.Parameter(torch.empty(self.nMutual).uniform_(-bound, bound)))
        self.mask = self.mask_index = self.negatives = None
        self._draws = 0

    def get_mask(self, x, mask_prob, mask_length, frames=None, seed=None):
        """x [B][T][nEncoder] with the chosen spans replaced by the mask embedding.  Stores the byte mask [B][T], the masked frames
        [B][M] and the negatives [B][M][K] for forward().  frames: the valid frames of every utterance (a sequence of B ints), None:
        all T, padding included, as the reference.  seed: None takes torch's initial seed plus the number of calls so far."""
        from . import cpc
        if x.dim() != 3 or x.shape[2] != self.nEncoder or x.dtype != torch.float32:
            raise _lib.W2LInvalidArgument("CPCCriterion.get_mask: x must be float32 [B][T][nEncoder]")
        _check_dev(x)
        B, T, _ = x.shape
        if seed is None:
            seed = torch.initial_seed() + self._draws
        self._draws += 1
        try:
            mask, index, neg = cpc.sample(B, T, mask_prob, int(mask_length), self.nNegative,
                                          None if frames is None else [int(f) for f in frames], seed)
        except ValueError as e:
            raise _lib.W2LInvalidArgument(str(e)) from None
        self.mask = torch.from_numpy(mask).to(x.device)
        self.mask_index = torch.from_numpy(index).to(x.device)
        self.negatives = torch.from_numpy(neg).to(x.device)
        return _CPCMask.apply(x, self.mask_embedding, self.mask)

    def num_mask(self):
        """masked frames of the last get_mask over the whole batch (the reference's numMask)"""
        return 0 if self.mask_index is None else int(self.mask_index.numel())

    def forward(self, enc, context):
        """loss [B]: enc [B][T][nEncoder] is the encoder output BEFORE masking (the targets), context [B][T][nContext] the context
        network's output on the masked input"""
        if self.mask_index is None:
            raise _lib.W2LInvalidArgument("CPCCriterion.forward: call get_mask first")
        for t, n, what in ((enc, self.nEncoder, "enc"), (context, self.nContext, "context")):
            if t.dim() != 3 or t.shape[2] != n or t.dtype != torch.float32:
                raise _lib.W2LInvalidArgument(f"CPCCriterion.forward: {what} must be float32 [B][T][{n}]")
        _check_dev(enc, context)
        if enc.shape[:2] != context.shape[:2] or tuple(enc.shape[:2]) != tuple(self.mask.shape):
            raise _lib.W2LInvalidArgument("CPCCriterion.forward: enc, context and the stored mask must agree in B and T")
        return _CPC.apply(enc, context, self.encoder_weight, self.encoder_bias, self.context_weight, self.context_bias,
                          self.mask_index, self.negatives, self.temperature)

    def viterbiPath(self, emission, inputSize=None):
        raise _lib.W2LError("CPCCriterion has no viterbiPath (the reference exits there)")

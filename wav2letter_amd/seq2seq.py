"""The teacher-forced training path of the reference's --criterion=seq2seq (Flashlight's Seq2SeqCriterion, vectorizedDecoder): an
embedding, a one-layer GRU, one round of encoder-decoder attention, a Linear and a label-smoothed cross entropy (DESIGN.md 3.34 is the
contract).  Composed from ops.embedding, ops.rnn, ops.s2s_attention, the fp32 Linear products and ops.s2s_cross_entropy; every one
of them is a HIP kernel behind the C ABI, and there is no other path.  The teacher-forcing draws are this project's seeded
splitmix64 stream (as wav2letter_amd/cpc.py), not ArrayFire's."""
import numpy as np
import torch

from . import _lib, ops
from .cpc import CpcRng
from .criterion import SequenceCriterion, _check_dev


def teacher_forcing(y, nClass, pctTeacherForcing, seed):
    """y [B][U] int (padding already read as eos) -> (y' int32, replaced bool): every entry, in row-major order, takes one draw r and is
    replaced when r % 100 >= pctTeacherForcing, then by a second draw % (nClass - 1).  pctTeacherForcing >= 100 makes no draws."""
    y = np.array(y, dtype=np.int32)
    replaced = np.zeros(y.shape, bool)
    if pctTeacherForcing >= 100:
        return y, replaced
    rng = CpcRng(seed)
    for b in range(y.shape[0]):
        for u in range(y.shape[1]):
            if rng.next() % 100 >= pctTeacherForcing:
                y[b, u], replaced[b, u] = rng.next() % (nClass - 1), True
    return y, replaced


class _Linear(torch.autograd.Function):
    """fl::Linear on w2l_linear_forward / _backward_data / _backward_weight_bias: x [M][K], w [K][N], bias [N]"""

    @staticmethod
    def forward(ctx, x, w, bias):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(x, w)
        return ops.linear_forward(x, w, bias.contiguous())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return ops.linear_backward(x, w, dy.contiguous())


class Seq2SeqCriterion(SequenceCriterion):
    """forward(enc [B][T][C], target [B][U]) -> (loss [B], alpha [B][U][T]); C = hiddenDim for attention="content" (keys = values =
    enc) and 2 hiddenDim for "keyvalue" (keys, then values).  Parameters in the reference's order: the embedding [nClass][hiddenDim],
    the GRU (one flat parameter, include/w2l_hip.h), the output Linear [hiddenDim][nClass] and its bias, the start embedding
    [hiddenDim].  Not built, and refused by name: input feeding, model / gumbel sampling, more than one attention round or RNN layer,
    the other attention and window kinds.  beamSearch and viterbiPath decode the trained model."""

    def __init__(self, nClass, hiddenDim, eos, attention="content", window=None, trainWithWindow=False, pctTeacherForcing=100,
                 labelSmooth=0.0, inputFeeding=False, samplingStrategy="rand", nAttnRound=1, nRnnLayer=1):
        super().__init__()
        refuse = _lib.W2LInvalidArgument
        if inputFeeding:
            raise refuse("Seq2SeqCriterion: input feeding is not built")
        if samplingStrategy != "rand":
            raise refuse(f"Seq2SeqCriterion: sampling strategy '{samplingStrategy}' is not built (rand only)")
        if nAttnRound != 1 or nRnnLayer != 1:
            raise refuse("Seq2SeqCriterion: more than one attention round or RNN layer is not built")
        if attention not in ("content", "keyvalue"):
            raise refuse(f"Seq2SeqCriterion: attention '{attention}' is not built (content, keyvalue)")
        if window is not None and (len(window) != 2 or window[0] != "softPretrain" or not float(window[1]) > 0):
            raise refuse(f"Seq2SeqCriterion: window {window!r} is not built (None or ('softPretrain', std > 0))")
        if nClass < 2 or not 0 <= eos < nClass or hiddenDim < 1 or not 0.0 <= labelSmooth < 1.0 or not 0 <= pctTeacherForcing <= 100:
            raise refuse("Seq2SeqCriterion: nClass >= 2, 0 <= eos < nClass, hiddenDim >= 1, labelSmooth in [0, 1), pctTeacherForcing in 0..100")
        self.nClass, self.hiddenDim, self.eos, self.attention = int(nClass), int(hiddenDim), int(eos), attention
        self.windowStd = None if window is None else float(window[1])
        self.trainWithWindow, self.pctTeacherForcing, self.labelSmooth = bool(trainWithWindow), int(pctTeacherForcing), float(labelSmooth)
        N, H = self.nClass, self.hiddenDim
        bound = H ** -0.5
        self.embedding = torch.nn.Parameter(torch.empty(N, H).uniform_(-bound, bound))
        self.rnn = torch.nn.Parameter(torch.empty(3 * H * (2 * H + 2)).uniform_(-bound, bound))
        self.linear_weight = torch.nn.Parameter(torch.empty(H, N).uniform_(-bound, bound))
        self.linear_bias = torch.nn.Parameter(torch.empty(N).uniform_(-bound, bound))
        self.start = torch.nn.Parameter(torch.empty(H).uniform_(-0.1, 0.1))
        self.replaced = None      # which decoder inputs the last training call replaced, [B][U] bool
        self._draws = 0

    def forward(self, enc, target, inputSizes=None, targetSizes=None, seed=None):
        """target: [B][U] integers, every row tgtLen valid tokens ending in eos, then padding (negative, or anything when targetSizes
        gives the lengths).  inputSizes: relative lengths of the utterances, keyLen = ceil(inputSizes / max(inputSizes) T).  seed: of
        the teacher-forcing draws; None takes torch's initial seed plus the number of training calls so far."""
        H, N = self.hiddenDim, self.nClass
        if enc.dim() != 3 or enc.dtype != torch.float32 or enc.shape[2] != (2 * H if self.attention == "keyvalue" else H):
            raise _lib.W2LInvalidArgument(f"Seq2SeqCriterion: enc must be float32 [B][T][{2 * H if self.attention == 'keyvalue' else H}]")
        _check_dev(enc)
        B, T, _ = enc.shape
        y = ops._host_i32(target)
        if y.ndim != 2 or y.shape[0] != B:
            raise _lib.W2LInvalidArgument("Seq2SeqCriterion: target must be [B][U]")
        U = y.shape[1]
        tl = (y >= 0).sum(1).astype(np.int32) if targetSizes is None else ops._host_i32(targetSizes).reshape(-1)
        if tl.shape != (B,) or tl.min() < 1 or tl.max() > U:
            raise _lib.W2LInvalidArgument("Seq2SeqCriterion: every target needs 1..U valid tokens")
        valid = np.arange(U)[None, :] < tl[:, None]
        if (y[valid] < 0).any() or (y[valid] >= N).any():
            raise _lib.W2LInvalidArgument("Seq2SeqCriterion: a target token lies outside 0..nClass-1")
        if inputSizes is None:
            kl = np.full(B, T, np.int32)
        else:
            sz = np.asarray(inputSizes.detach().cpu() if torch.is_tensor(inputSizes) else inputSizes, dtype=np.float64).reshape(-1)
            if sz.shape != (B,) or not (sz > 0).all():
                raise _lib.W2LInvalidArgument("Seq2SeqCriterion: inputSizes must hold B positive sizes")
            kl = np.ceil(sz / sz.max() * T).astype(np.int32).clip(1, T)
        # 1. decoder input: the start embedding, then the embedding of the previous token (teacher forcing, with random replacement)
        prev = np.where(valid, y, self.eos).astype(np.int32)
        if self.training and self.pctTeacherForcing < 100:
            if seed is None:
                seed = torch.initial_seed() + self._draws
            self._draws += 1
            prev, self.replaced = teacher_forcing(prev, N, self.pctTeacherForcing, seed)
        else:
            self.replaced = np.zeros((B, U), bool)
        tokens = np.concatenate([np.full((B, 1), -1, np.int32), prev[:, :U - 1]], axis=1)
        x = ops.embedding(tokens, self.embedding, self.start)
        # 2. the recurrence, 3. attention (o = h + context), 4. the output projection, 5. the loss
        h = ops.rnn(x, self.rnn, "gru", H, train=torch.is_grad_enabled())
        std = self.windowStd if (self.windowStd is not None and (not self.training or self.trainWithWindow)) else None
        o, alpha = ops.s2s_attention(h, enc, kl, tl, self.attention == "keyvalue", std, add_query=True)
        z = _Linear.apply(o.view(B * U, H), self.linear_weight, self.linear_bias)
        loss = ops.s2s_cross_entropy(z, np.where(valid, y, -1).reshape(-1), self.labelSmooth if self.training else 0.0, B=B)
        return loss, alpha

    def _key_len(self, enc, inputSizes):
        B, T, _ = enc.shape
        if inputSizes is None:
            return np.full(B, T, np.int32)
        sz = np.asarray(inputSizes.detach().cpu() if torch.is_tensor(inputSizes) else inputSizes, dtype=np.float64).reshape(-1)
        if sz.shape != (B,) or not (sz > 0).all():
            raise _lib.W2LInvalidArgument("Seq2SeqCriterion: inputSizes must hold B positive sizes")
        return np.ceil(sz / sz.max() * T).astype(np.int32).clip(1, T)

    @torch.no_grad()
    def beamSearch(self, enc, inputSizes=None, beam=1, beam_token=None, threshold=None, eos_score=0.0, attention_threshold=None,
                   temperature=1.0, max_len=120, nbest=1, lm=None, **refused):
        """token beam search over the step-by-step decoder (ops.s2s_decode; the reference's LexiconFreeSeq2SeqDecoder)
        -> (tokens [B][nbest][max_len], -1 behind the end and eos included when reached; lengths [B][nbest]; scores [B][nbest]).
        lm=<NGramLM over the nClass classes>, lm_weight= (or lmweight=): the n-gram LM fused into the search; a
        fourth value is then the hypotheses' unweighted LM scores [B][nbest].
        beam_token None: min(nClass, 64); threshold None: no beam threshold; attention_threshold None: off.  The
        decoder applies NO window: the recipe's softPretrain window is a pre-training device, and its centre u keyLen / tgtLen has no
        meaning without a target.  Refused by name: LM fusion without lm=, hard and soft selection."""
        refuse = _lib.W2LInvalidArgument
        names = {"lm_weight": "LM fusion (lm_weight) needs lm=", "lmweight": "LM fusion (lmweight) needs lm=",
                 "hardselection": "hardselection is not built", "softselection": "softselection is not built",
                 "hard_selection": "hardselection is not built", "soft_selection": "softselection is not built"}
        for k, v in refused.items():
            if k not in names:
                raise TypeError(f"Seq2SeqCriterion.beamSearch: unknown option '{k}'")
            if k in ("lm_weight", "lmweight") and (lm is not None or not v):
                continue
            raise refuse(f"Seq2SeqCriterion.beamSearch: {names[k]}")
        if lm is not None and lm.num_tokens != self.nClass:
            raise refuse(f"Seq2SeqCriterion.beamSearch: the LM has {lm.num_tokens} tokens, nClass is {self.nClass}")
        lm_weight = float(refused.get("lm_weight", refused.get("lmweight", 0.0)))
        _check_dev(enc)
        params = [p.detach() for p in (self.embedding, self.start, self.rnn, self.linear_weight, self.linear_bias)]
        return ops.s2s_decode(params, enc, self._key_len(enc, inputSizes), self.attention == "keyvalue", eos=self.eos, beam=beam,
                              beam_token=beam_token, threshold=threshold, eos_score=eos_score, attention_threshold=attention_threshold,
                              temperature=temperature, max_len=max_len, nbest=nbest, lm=lm, lm_weight=lm_weight)

    def viterbiPath(self, enc, inputSizes=None, max_len=120):
        """greedy step-by-step decoding, the beam-1 case of beamSearch -> tokens [B][max_len] int32, -1 behind the end"""
        return self.beamSearch(enc, inputSizes, beam=1, beam_token=1, max_len=max_len)[0][:, 0]

    def prettyString(self):
        return f"Seq2SeqCriterion(nClass={self.nClass}, hiddenDim={self.hiddenDim}, attention={self.attention})"


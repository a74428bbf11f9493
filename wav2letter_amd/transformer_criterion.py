"""The teacher-forced training path of the reference's --criterion=transformer (Flashlight's TransformerCriterion, vectorizedDecoder): an
embedding, nLayer masked Transformer blocks, one round of encoder-decoder attention, a Linear and a label-smoothed cross entropy
(DESIGN.md 3.37 is the contract).  The hot piece is ops.attn_causal, the fused causal self-attention kernel; the rest is composed from
ops.embedding, the fp32 Linear products, ops.residual_layernorm_forward / layernorm_backward, ops.s2s_attention and
ops.s2s_cross_entropy.  Every one of them is a HIP kernel behind the C ABI, and there is no other path.  The random draws are this
project's seeded splitmix64 stream (wav2letter_amd/cpc.py), not ArrayFire's."""
import numpy as np
import torch

from . import _lib, ops
from .cpc import CpcRng
from .criterion import SequenceCriterion, _check_dev
from .seq2seq import _Linear, teacher_forcing

_GOLDEN, _M64 = 0x9E3779B97F4A7C15, (1 << 64) - 1
HEAD_WIDTHS = tuple(range(32, 257, 32))     # what w2l_attn_causal_* takes


def layer_drop(nLayer, pLayerDrop, seed, draws_before=0):
    """[nLayer] bool, True = the block is dropped in this call: one draw per block from the splitmix64 stream of `seed`, continued behind
    `draws_before` earlier draws (the teacher-forcing ones); dropped when the draw's upper 53 bits, as a fraction, lie below pLayerDrop"""
    rng = CpcRng((int(seed) + draws_before * _GOLDEN) & _M64)
    return np.array([(rng.next() >> 11) * 2.0 ** -53 < pLayerDrop for _ in range(nLayer)], bool)


class _Mlp(torch.autograd.Function):
    """relu(h w1 + b1) w2 + b2; the ReLU's mask rides in the second product's data gradient"""

    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2):
        h, w1, w2 = h.contiguous(), w1.contiguous(), w2.contiguous()
        u = ops.linear_forward(h, w1, b1.contiguous(), relu=True)
        ctx.save_for_backward(h, u, w1, w2)
        return ops.linear_forward(u, w2, b2.contiguous())

    @staticmethod
    def backward(ctx, dy):
        h, u, w1, w2 = ctx.saved_tensors
        du, dw2, db2 = ops.linear_backward(u, w2, dy.contiguous(), mask_src=u, mask_scale=1.0)
        dh, dw1, db1 = ops.linear_backward(h, w1, du)
        return dh, dw1, db1, dw2, db2


class _ResidualLayerNorm(torch.autograd.Function):
    """LayerNorm(a + x) over every row, scalar affine; x None: LayerNorm(a).  No dropout: the reference's block has none on its
    residual branches (TransformerCPC.cpp:166-176), as the TR layer of host/net.cpp"""

    @staticmethod
    def forward(ctx, a, x, gb):
        a, gb, x = a.contiguous(), gb.contiguous(), None if x is None else x.contiguous()
        y, r, mr = ops.residual_layernorm_forward(a, x, gb, a.shape[0], 1e-5)
        ctx.has_x = x is not None
        ctx.save_for_backward(r, gb, mr)
        return y

    @staticmethod
    def backward(ctx, dy):
        r, gb, mr = ctx.saved_tensors
        dr, dgb, _ = ops.layernorm_backward(r, dy.contiguous(), gb, mr, r.shape[0])
        return dr, (dr if ctx.has_x else None), dgb


class TransformerCriterion(SequenceCriterion):
    """forward(enc [B][T][C], target [B][U]) -> (loss [B], alpha [B][U][T]); C = hiddenDim for attention="content" and 2 hiddenDim for
    "keyvalue", as Seq2SeqCriterion.  Parameters: the embedding [nClass][hiddenDim]; per block (`blocks[l]`), in the layouts the kernels
    read, so that no call copies a weight: the position table [2 maxDecoderOutputLen - 1][d], w1, b1, w2, b2 (MLP width 4 hiddenDim),
    wqkv [hiddenDim][3 hiddenDim] = wq | wk | wv and bqkv, wf, bf and the two LayerNorms' (gamma, beta); the output Linear
    [hiddenDim][nClass] and its bias; the start embedding [hiddenDim].  reference_params(l) gives the block's 15 tensors in
    oracle/transformer_oracle.py's tr_param_shapes order and layouts, as views.  Not built, and refused by name: the other attention and window kinds, the step-by-step decoder."""

    def __init__(self, nClass, hiddenDim, eos, nLayer, attention="content", window=None, trainWithWindow=False, pctTeacherForcing=100,
                 labelSmooth=0.0, pDropout=0.0, pLayerDrop=0.0, maxDecoderOutputLen=120, nHeads=4):
        super().__init__()
        refuse = _lib.W2LInvalidArgument
        if attention not in ("content", "keyvalue"):
            raise refuse(f"TransformerCriterion: attention '{attention}' is not built (content, keyvalue)")
        if window is not None and (len(window) != 2 or window[0] != "softPretrain" or not float(window[1]) > 0):
            raise refuse(f"TransformerCriterion: window {window!r} is not built (None or ('softPretrain', std > 0))")
        if nClass < 2 or not 0 <= eos < nClass or hiddenDim < 1 or nLayer < 1 or nHeads < 1 or not 0.0 <= labelSmooth < 1.0 or \
                not 0 <= pctTeacherForcing <= 100 or not 0.0 <= pDropout < 1.0 or not 0.0 <= pLayerDrop < 1.0 or maxDecoderOutputLen < 1:
            raise refuse("TransformerCriterion: nClass >= 2, 0 <= eos < nClass, hiddenDim, nLayer, nHeads, maxDecoderOutputLen >= 1, "
                         "labelSmooth, pDropout, pLayerDrop in [0, 1), pctTeacherForcing in 0..100")
        if hiddenDim % nHeads:
            raise refuse(f"TransformerCriterion: hiddenDim {hiddenDim} is no multiple of nHeads {nHeads}")
        if hiddenDim // nHeads not in HEAD_WIDTHS or hiddenDim > 1024:
            raise refuse(f"TransformerCriterion: head width {hiddenDim // nHeads} is not built (a multiple of 32 up to 256, hiddenDim <= 1024)")
        self.nClass, self.hiddenDim, self.eos, self.nLayer, self.nHeads, self.attention = int(nClass), int(hiddenDim), int(eos), int(nLayer), int(nHeads), attention
        self.windowStd = None if window is None else float(window[1])
        self.trainWithWindow, self.pctTeacherForcing, self.labelSmooth = bool(trainWithWindow), int(pctTeacherForcing), float(labelSmooth)
        self.pDropout, self.pLayerDrop, self.maxDecoderOutputLen = float(pDropout), float(pLayerDrop), int(maxDecoderOutputLen)
        N, H, d, csz = self.nClass, self.hiddenDim, self.hiddenDim // self.nHeads, self.maxDecoderOutputLen
        bound = H ** -0.5
        uni = lambda *shape, b=bound: torch.nn.Parameter(torch.empty(*shape).uniform_(-b, b))
        self.embedding = uni(N, H)
        self.blocks = torch.nn.ModuleList()
        for _ in range(self.nLayer):
            ps = [uni(2 * csz - 1, d, b=d ** -0.5)]
            for i, o in ((H, 4 * H), (4 * H, H), (H, 3 * H), (H, H)):
                ps += [uni(i, o, b=i ** -0.5), uni(o, b=i ** -0.5)]
            ps += [torch.nn.Parameter(torch.tensor([1.0, 0.0])), torch.nn.Parameter(torch.tensor([1.0, 0.0]))]
            self.blocks.append(torch.nn.ParameterList(ps))
        self.linear_weight, self.linear_bias = uni(H, N), uni(N)
        self.start = uni(H, b=0.1)
        self.replaced = None      # which decoder inputs the last training call replaced, [B][U] bool
        self.dropped = None       # which blocks the last call dropped, [nLayer] bool
        self._draws = 0

    def reference_params(self, layer):
        """the block's parameters in tr_param_shapes order and layouts, as views of the stored ones"""
        pos, w1, b1, w2, b2, wqkv, bqkv, wf, bf, g1, g2 = self.blocks[layer]
        H = self.hiddenDim
        qkv = [t for n in range(3) for t in (wqkv[:, n * H:(n + 1) * H], bqkv[n * H:(n + 1) * H])]
        return [pos.t(), w1, b1, w2, b2, *qkv, wf, bf, g1, g2]

    def _block(self, x, ps, tl, B, U, f, seed, layer):
        """one post-LayerNorm block on rows x [B U][H]: f = 0 (the block is dropped) leaves the two LayerNorms and launches nothing else.
        Dropout acts on the attention probabilities only."""
        H, p = self.hiddenDim, self.pDropout if self.training else 0.0
        pos, w1, b1, w2, b2, wqkv, bqkv, wf, bf, g1, g2 = ps
        if not f:
            return _ResidualLayerNorm.apply(_ResidualLayerNorm.apply(x, None, g1), None, g2)
        qkv = _Linear.apply(x, wqkv, bqkv).view(B, U, 3 * H)
        o = ops.attn_causal(qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], pos, tl, self.nHeads, self.maxDecoderOutputLen - 1,
                            (H // self.nHeads) ** -0.5, p, seed, layer)
        h = _ResidualLayerNorm.apply(_Linear.apply(o.view(B * U, H), wf, bf), x, g1)
        return _ResidualLayerNorm.apply(_Mlp.apply(h, w1, b1, w2, b2), h, g2)

    def forward(self, enc, target, inputSizes=None, targetSizes=None, seed=None):
        """target, inputSizes, targetSizes: as Seq2SeqCriterion.forward.  seed: of the teacher-forcing draws, the layer-drop draws behind
        them and the dropout masks; None takes torch's initial seed plus the number of training calls so far."""
        H, N, who = self.hiddenDim, self.nClass, "TransformerCriterion"
        if enc.dim() != 3 or enc.dtype != torch.float32 or enc.shape[2] != (2 * H if self.attention == "keyvalue" else H):
            raise _lib.W2LInvalidArgument(f"{who}: enc must be float32 [B][T][{2 * H if self.attention == 'keyvalue' else H}]")
        B, T, _ = enc.shape
        y = ops._host_i32(target)
        if y.ndim != 2 or y.shape[0] != B:
            raise _lib.W2LInvalidArgument(f"{who}: target must be [B][U]")
        U = y.shape[1]
        if U > self.maxDecoderOutputLen:
            raise _lib.W2LInvalidArgument(f"{who}: U = {U} targets exceed maxDecoderOutputLen = {self.maxDecoderOutputLen}")
        tl = (y >= 0).sum(1).astype(np.int32) if targetSizes is None else ops._host_i32(targetSizes).reshape(-1)
        if tl.shape != (B,) or tl.min() < 1 or tl.max() > U:
            raise _lib.W2LInvalidArgument(f"{who}: every target needs 1..U valid tokens")
        valid = np.arange(U)[None, :] < tl[:, None]
        if (y[valid] < 0).any() or (y[valid] >= N).any():
            raise _lib.W2LInvalidArgument(f"{who}: a target token lies outside 0..nClass-1")
        if inputSizes is None:
            kl = np.full(B, T, np.int32)
        else:
            sz = np.asarray(inputSizes.detach().cpu() if torch.is_tensor(inputSizes) else inputSizes, dtype=np.float64).reshape(-1)
            if sz.shape != (B,) or not (sz > 0).all():
                raise _lib.W2LInvalidArgument(f"{who}: inputSizes must hold B positive sizes")
            kl = np.ceil(sz / sz.max() * T).astype(np.int32).clip(1, T)
        _check_dev(enc)
        # the draws of this call: teacher forcing, then one per block
        prev = np.where(valid, y, self.eos).astype(np.int32)
        self.replaced, self.dropped = np.zeros((B, U), bool), np.zeros(self.nLayer, bool)
        if self.training:
            if seed is None:
                seed = torch.initial_seed() + self._draws
            self._draws += 1
            if self.pctTeacherForcing < 100:
                prev, self.replaced = teacher_forcing(prev, N, self.pctTeacherForcing, seed)
            if self.pLayerDrop > 0:
                tf_draws = B * U + int(self.replaced.sum()) if self.pctTeacherForcing < 100 else 0
                self.dropped = layer_drop(self.nLayer, self.pLayerDrop, seed, tf_draws)
        seed32 = int(seed or 0) & 0xFFFFFFFF
        # 1. decoder input, 2. the blocks, 3. encoder-decoder attention (the summary alone goes on), 4. the output projection and the loss
        tokens = np.concatenate([np.full((B, 1), -1, np.int32), prev[:, :U - 1]], axis=1)
        x = ops.embedding(tokens, self.embedding, self.start).view(B * U, H)
        for layer, ps in enumerate(self.blocks):
            x = self._block(x, list(ps), tl, B, U, not self.dropped[layer], seed32, layer)
        std = self.windowStd if (self.windowStd is not None and (not self.training or self.trainWithWindow)) else None
        o, alpha = ops.s2s_attention(x.view(B, U, H), enc, kl, tl, self.attention == "keyvalue", std, add_query=False)
        z = _Linear.apply(o.view(B * U, H), self.linear_weight, self.linear_bias)
        loss = ops.s2s_cross_entropy(z, np.where(valid, y, -1).reshape(-1), self.labelSmooth if self.training else 0.0, B=B)
        return loss, alpha

    def beamSearch(self, *args, **kwargs):
        raise _lib.W2LUnsupported("TransformerCriterion.beamSearch: the step-by-step decoder of this criterion is not built")

    def viterbiPath(self, *args, **kwargs):
        raise _lib.W2LUnsupported("TransformerCriterion.viterbiPath: the step-by-step decoder of this criterion is not built")

    def prettyString(self):
        return f"TransformerCriterion(nClass={self.nClass}, hiddenDim={self.hiddenDim}, nLayer={self.nLayer}, nHeads={self.nHeads}, attention={self.attention})"

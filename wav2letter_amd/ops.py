"""Thin torch-tensor front-ends of the network-operator C ABI (include/w2l_hip.h
section 2).  Used by tests and by the Python side of bench.py; the C++ host
(wav2letter_amd/csrc/host) calls the same kernels directly.  Frame-major
activations: [B][T][H][C]."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, RnnDesc, S2sAttnDesc, check


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def gemm(A, B, a_kcontig=True, b_kcontig=False, bias=None, relu=False, splitk=1):
    """C = op(A) op(B): A [M][K] if a_kcontig else [K][M]; B [N][K] if b_kcontig else [K][N]"""
    M, K = (A.shape if a_kcontig else A.shape[::-1])
    N = B.shape[0] if b_kcontig else B.shape[1]
    Cm = torch.empty(M, N, device=A.device, dtype=torch.float32)
    check(_lib.lib().w2l_gemm_f32(M, N, K, _p(A), A.stride(0), int(a_kcontig), _p(B), B.stride(0), int(b_kcontig),
                                  _p(Cm), N, _p(bias), int(relu), splitk, _s()), "gemm")
    return Cm


def linear_forward(x, w, bias=None, relu=False):
    M, K = x.shape
    N = w.shape[1]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_linear_forward(M, K, N, _p(x), _p(w), _p(bias), _p(y), int(relu), _s()), "linear_forward")
    return y


def weightnorm_forward(v, g):
    """fl::WeightNorm on the internal [K][Nout] weight layout: w = v * g / ||v|| per column; returns (w, norm)"""
    K, N = v.shape
    w = torch.empty_like(v)
    norm = torch.empty(N, device=v.device, dtype=torch.float32)
    check(_lib.lib().w2l_weightnorm_forward(_p(v), _p(g), _p(w), _p(norm), K, N, _s()), "weightnorm_forward")
    return w, norm


def weightnorm_backward(v, g, norm, dw):
    K, N = v.shape
    dv = torch.empty_like(v)
    dg = torch.empty(N, device=v.device, dtype=torch.float32)
    dot = torch.empty(N, device=v.device, dtype=torch.float32)
    check(_lib.lib().w2l_weightnorm_backward(_p(v), _p(g), _p(norm), _p(dw), _p(dv), _p(dg), _p(dot), K, N, _s()), "weightnorm_backward")
    return dv, dg


def colsum(x):
    """out[n] = sum_m x[m][n] (bias gradient): deterministic two-pass sum"""
    M, N = x.shape
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_colsum(_p(x), _p(out), M, N, _s()), "colsum")
    return out


def linear_backward(x, w, dy, mask_src=None, mask_scale=1.0):
    M, K = x.shape
    N = w.shape[1]
    dx = torch.empty_like(x)
    dw = torch.empty_like(w)
    db = torch.empty(N, device=x.device, dtype=torch.float32)
    L = _lib.lib()
    check(L.w2l_linear_backward_data(M, K, N, _p(dy), _p(w), _p(dx), 0, _p(mask_src), mask_scale, _s()), "linear_bwd_data")
    check(L.w2l_linear_backward_weight_bias(M, K, N, _p(x), _p(dy), _p(dw), _p(db), _s()), "linear_bwd_weight_bias")
    return dx, dw, db


def conv_desc(x, w, stride, padl, padr):
    B, T, H, Cin = x.shape
    kw, _, Cout = w.shape
    return ConvDesc(B, T, H, Cin, Cout, kw, stride, padl, padr)


def conv_forward(x, w, bias=None, stride=1, padl=0, padr=0, relu=False):
    """x [B][T][H][Cin], w [kw][Cin][Cout] -> y [B][To][H][Cout]"""
    d = conv_desc(x, w, stride, padl, padr)
    To = _lib.lib().w2l_conv_out_len(d.T, d.kw, stride, padl, padr)
    y = torch.empty(d.B, To, d.H, d.Cout, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_conv_forward(C.byref(d), _p(x), _p(w), _p(bias), _p(y), int(relu), _s()), "conv_forward")
    return y


def conv_backward(x, w, dy, stride=1, padl=0, padr=0, need_dx=True):
    d = conv_desc(x, w, stride, padl, padr)
    L = _lib.lib()
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w)
    db = torch.empty(d.Cout, device=x.device, dtype=torch.float32)
    if need_dx:
        check(L.w2l_conv_backward_data(C.byref(d), _p(dy), _p(w), _p(dx), 0, _s()), "conv_bwd_data")
    check(L.w2l_conv_backward_filter(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _s()), "conv_bwd_filter")
    return dx, dw, db


def conv_depthwise_desc(x, w, stride=1, padl=0, padr=0):
    B, T, H, Cin = x.shape
    kw, Cout = w.shape
    return ConvDesc(B, T, H, Cin, Cout, kw, stride, padl, padr)


def conv_depthwise_forward(x, w, bias=None, stride=1, padl=0, padr=0):
    """depthwise (groups == C) convolution over time: x [B][T][H][C], w [kw][C], bias [C] -> y [B][To][H][C]"""
    d = conv_depthwise_desc(x, w, stride, padl, padr)
    To = max(_lib.lib().w2l_conv_out_len(d.T, d.kw, stride, padl, padr), 0)
    y = torch.empty(d.B, To, d.H, d.Cout, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_conv_depthwise_forward(C.byref(d), _p(x), _p(w), _p(bias), _p(y), _s()), "conv_depthwise_forward")
    return y


def conv_depthwise_backward(x, w, dy, stride=1, padl=0, padr=0, need_dx=True, need_dbias=True):
    """-> (dx or None, dw [kw][C], dbias [C] or None); the filter gradient is run-to-run deterministic (no atomics)"""
    d = conv_depthwise_desc(x, w, stride, padl, padr)
    L = _lib.lib()
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w)
    db = torch.empty(d.Cout, device=x.device, dtype=torch.float32) if need_dbias else None
    ws = torch.empty(max(L.w2l_conv_depthwise_workspace_floats(C.byref(d)), 1), device=x.device, dtype=torch.float32)
    if need_dx:
        check(L.w2l_conv_depthwise_backward_data(C.byref(d), _p(dy), _p(w), _p(dx), _s()), "conv_depthwise_bwd_data")
    check(L.w2l_conv_depthwise_backward_filter(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(ws), _s()), "conv_depthwise_bwd_filter")
    return dx, dw, db


def swish_forward(x, beta=1.0):
    """fl::Swish: y = x * sigmoid(beta * x)"""
    y = torch.empty_like(x)
    check(_lib.lib().w2l_swish_forward(_p(x), _p(y), x.numel(), beta, _s()), "swish_forward")
    return y


def swish_backward(x, dy, beta=1.0, out=None):
    """dx = dy * (s + beta x s (1 - s)), s = sigmoid(beta x); out may be dy itself"""
    dx = torch.empty_like(dy) if out is None else out
    check(_lib.lib().w2l_swish_backward(_p(x), _p(dy), _p(dx), x.numel(), beta, _s()), "swish_backward")
    return dx


RNN_MODES = {"relu": 0, "tanh": 1, "lstm": 2, "gru": 3}


def rnn_desc(x, mode, H, layers=1, bidirectional=False, dropout=0.0, train=False, seed=0, rng_stream=0):
    """x [B][T][I] (dense); mode: a key of RNN_MODES or its number"""
    B, T, I = x.shape
    dirs = 2 if bidirectional else 1
    return RnnDesc(RNN_MODES.get(mode, mode), I, H, layers, dirs, B, T, I, H * dirs, int(train), dropout, seed, rng_stream)


def rnn_param_count(mode, I, H, layers=1, bidirectional=False):
    d = RnnDesc(RNN_MODES.get(mode, mode), I, H, layers, 2 if bidirectional else 1, 1, 1, I, H * (2 if bidirectional else 1), 0, 0.0, 0, 0)
    return int(_lib.lib().w2l_rnn_param_count(C.byref(d)))


def rnn_forward(d, x, params):
    """fl::RNN forward (w2l_rnn_forward) -> (y [B][T][H dirs], workspace); the workspace is what rnn_backward needs when d.train"""
    L = _lib.lib()
    nbytes = L.w2l_rnn_workspace_size(C.byref(d))
    ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
    y = torch.empty(d.B, d.T, d.ldy, device=x.device, dtype=torch.float32)
    check(L.w2l_rnn_forward(C.byref(d), _p(x), _p(params), _p(y), _p(ws), nbytes, _s()), "rnn_forward")
    return y, ws


def rnn_backward(d, x, params, y, dy, ws, need_dx=True):
    """-> (dx or None, dparams), from the descriptor, operands and workspace of a training rnn_forward"""
    dx = torch.empty_like(x) if need_dx else None
    dparams = torch.empty_like(params)
    check(_lib.lib().w2l_rnn_backward(C.byref(d), _p(x), _p(params), _p(y), _p(dy), _p(dx), _p(dparams), _p(ws), ws.numel() * 4, _s()), "rnn_backward")
    return dx, dparams


class _Rnn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, d):
        x, params = x.contiguous(), params.contiguous()
        y, ws = rnn_forward(d, x, params)
        ctx.d, ctx.ws = d, ws
        ctx.save_for_backward(x, params, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, params, y = ctx.saved_tensors
        dx, dparams = rnn_backward(ctx.d, x, params, y, dy.contiguous(), ctx.ws, ctx.needs_input_grad[0])
        return dx, dparams, None


def rnn(x, params, mode, H, layers=1, bidirectional=False, dropout=0.0, train=True, seed=0, rng_stream=0):
    """fl::RNN as a differentiable torch op over the C ABI: x [B][T][I], params flat (rnn_param_count floats, the order of
    include/w2l_hip.h) -> y [B][T][H dirs].  train=False: no dropout and no backward."""
    return _Rnn.apply(x, params, rnn_desc(x, mode, H, layers, bidirectional, dropout, train, seed, rng_stream))


def _host_i32(a):
    """lengths, targets and tokens of the seq2seq kernels are HOST int32 arrays (the C ABI checks them before its first launch)"""
    return np.ascontiguousarray((a.detach().cpu() if torch.is_tensor(a) else a), dtype=np.int32)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


class _S2sAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, enc, key_len, tgt_len, keyvalue, window_std, add_query):
        if h.dim() != 3 or enc.dim() != 3 or h.dtype != torch.float32 or enc.dtype != torch.float32 or enc.shape[0] != h.shape[0]:
            raise _lib.W2LInvalidArgument("s2s_attention: h [B][U][H] and enc [B][T][C] float32")
        h, enc = h.contiguous(), enc.contiguous()
        (B, U, H), (_, T, Cc) = h.shape, enc.shape
        if Cc != (2 * H if keyvalue else H):
            raise _lib.W2LInvalidArgument(f"s2s_attention: enc must have {'2 H' if keyvalue else 'H'} = {2 * H if keyvalue else H} columns, got {Cc}")
        kl, tl = _host_i32(key_len), _host_i32(tgt_len)
        if kl.shape != (B,) or tl.shape != (B,):
            raise _lib.W2LInvalidArgument("s2s_attention: key_len and tgt_len must hold B lengths")
        d = S2sAttnDesc(B, U, T, H, Cc, float(window_std or 0.0), int(bool(add_query)))
        L = _lib.lib()
        out, alpha = torch.empty_like(h), torch.empty(B, U, T, device=h.device, dtype=torch.float32)
        nbytes = L.w2l_s2s_attn_workspace_size(C.byref(d), 0)
        ws = _ws(nbytes, h.device)
        k = enc.data_ptr()
        check(L.w2l_s2s_attn_forward(C.byref(d), _p(h), k, k + 4 * H * int(keyvalue), kl.ctypes.data, tl.ctypes.data, _p(out), _p(alpha),
                                     _p(ws), nbytes, _s()), "s2s_attn_forward")
        ctx.d, ctx.kl, ctx.tl, ctx.keyvalue = d, kl, tl, keyvalue
        ctx.save_for_backward(h, enc, alpha)
        ctx.set_materialize_grads(False)
        return out, alpha

    @staticmethod
    def backward(ctx, dout, dalpha):
        h, enc, alpha = ctx.saved_tensors
        d, L = ctx.d, _lib.lib()
        dout = torch.zeros_like(h) if dout is None else dout.contiguous()
        dalpha = None if dalpha is None else dalpha.contiguous()
        dh, denc = torch.empty_like(h), torch.empty_like(enc)
        nbytes = L.w2l_s2s_attn_workspace_size(C.byref(d), 1)
        ws = _ws(nbytes, h.device)
        k, dk = enc.data_ptr(), denc.data_ptr()
        off = 4 * d.H * int(ctx.keyvalue)
        check(L.w2l_s2s_attn_backward(C.byref(d), _p(h), k, k + off, ctx.kl.ctypes.data, ctx.tl.ctypes.data, _p(alpha), _p(dout), _p(dalpha),
                                      _p(dh), dk, dk + off, _p(ws), nbytes, _s()), "s2s_attn_backward")
        return dh, denc, None, None, None, None, None


def s2s_attention(h, enc, key_len, tgt_len, keyvalue=False, window_std=None, add_query=False):
    """encoder-decoder attention of the seq2seq criterion (w2l_s2s_attn_*): h [B][U][H] against enc [B][T][C] -- keys
    the columns 0..H-1 and values H..2H-1 when keyvalue (C = 2 H), else keys = values = enc (C = H) -- with key_len [B] valid keys,
    the soft window of width window_std around u key_len / tgt_len (None: no window) -> (context [B][U][H], + h when add_query;
    alpha [B][U][T]).  Differentiable in h and enc, through both results."""
    return _S2sAttention.apply(h, enc, key_len, tgt_len, bool(keyvalue), window_std, add_query)


def s2s_xent_forward(z, target, eps, row_utt=None, B=None):
    """w2l_s2s_xent_forward: z [M][N], target [M] host (-1: the row counts nothing) -> (loss [B], lse [M])"""
    M, N = z.shape
    B = int(B if B is not None else max(row_utt) + 1)
    L = _lib.lib()
    lse, loss = torch.empty(M, device=z.device, dtype=torch.float32), torch.empty(B, device=z.device, dtype=torch.float32)
    nbytes = L.w2l_s2s_xent_workspace_size(M, B)
    ws = _ws(nbytes, z.device)
    check(L.w2l_s2s_xent_forward(M, N, B, _p(z), target.ctypes.data, None if row_utt is None else row_utt.ctypes.data, eps, _p(lse), _p(loss),
                                 _p(ws), nbytes, _s()), "s2s_xent_forward")
    return loss, lse


def s2s_xent_backward(z, lse, target, eps, g, row_utt=None, out=None):
    """w2l_s2s_xent_backward -> dz [M][N]; out may be z itself"""
    M, N = z.shape
    B = g.numel()
    L = _lib.lib()
    dz = torch.empty_like(z) if out is None else out
    nbytes = L.w2l_s2s_xent_workspace_size(M, B)
    ws = _ws(nbytes, z.device)
    check(L.w2l_s2s_xent_backward(M, N, B, _p(z), _p(lse), target.ctypes.data, None if row_utt is None else row_utt.ctypes.data, eps, _p(g),
                                  _p(dz), _p(ws), nbytes, _s()), "s2s_xent_backward")
    return dz


class _S2sXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, target, eps, row_utt, B):
        z = z.contiguous()
        loss, lse = s2s_xent_forward(z, target, eps, row_utt, B)
        ctx.target, ctx.eps, ctx.row_utt = target, eps, row_utt
        ctx.save_for_backward(z, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, lse = ctx.saved_tensors
        return s2s_xent_backward(z, lse, ctx.target, ctx.eps, g.contiguous(), ctx.row_utt), None, None, None, None


def s2s_cross_entropy(z, target, eps=0.0, row_utt=None, B=None):
    """label-smoothed cross entropy summed per utterance (w2l_s2s_xent_*): z [M][N] float32, target [M] integers with
    -1 for a row that counts nothing, row_utt [M] the utterance of every row, non-decreasing (None: M / B rows each) -> loss [B]"""
    if z.dim() != 2 or z.dtype != torch.float32:
        raise _lib.W2LInvalidArgument("s2s_cross_entropy: z must be float32 [M][N]")
    target = _host_i32(target).reshape(-1)
    row_utt = None if row_utt is None else _host_i32(row_utt).reshape(-1)
    if target.shape[0] != z.shape[0] or (row_utt is not None and row_utt.shape != target.shape) or (row_utt is None and B is None):
        raise _lib.W2LInvalidArgument("s2s_cross_entropy: one target (and one row_utt, or B) per row of z")
    return _S2sXent.apply(z, target, float(eps), row_utt, B)


def embedding_forward(tokens, E, start):
    M, (N, H), L = tokens.shape[0], E.shape, _lib.lib()
    x = torch.empty(M, H, device=E.device, dtype=torch.float32)
    nbytes = L.w2l_embedding_workspace_size(M, N)
    ws = _ws(nbytes, E.device)
    check(L.w2l_embedding_forward(M, N, H, tokens.ctypes.data, _p(E), _p(start), _p(x), _p(ws), nbytes, _s()), "embedding_forward")
    return x


def embedding_backward(tokens, dx, N):
    """-> (dE [N][H], dstart [H]): position order inside every row, rows nobody holds are zero; no atomics"""
    (M, H), L = dx.shape, _lib.lib()
    dE, ds = torch.empty(N, H, device=dx.device, dtype=torch.float32), torch.empty(H, device=dx.device, dtype=torch.float32)
    nbytes = L.w2l_embedding_workspace_size(M, N)
    ws = _ws(nbytes, dx.device)
    check(L.w2l_embedding_backward(M, N, H, tokens.ctypes.data, _p(dx), _p(dE), _p(ds), _p(ws), nbytes, _s()), "embedding_backward")
    return dE, ds


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, start, tokens):
        ctx.tokens, ctx.N = tokens, E.shape[0]
        return embedding_forward(tokens, E.contiguous(), start.contiguous())

    @staticmethod
    def backward(ctx, dx):
        dE, ds = embedding_backward(ctx.tokens, dx.contiguous(), ctx.N)
        return dE, ds, None


def embedding(tokens, E, start):
    """token embedding (w2l_embedding_*): tokens, any shape of integers on the host, -1 = the start embedding ->
    x [*tokens.shape][H] = E[token] or start.  Differentiable in E [N][H] and start [H]."""
    if E.dim() != 2 or start.dim() != 1 or start.shape[0] != E.shape[1] or E.dtype != torch.float32 or start.dtype != torch.float32:
        raise _lib.W2LInvalidArgument("embedding: E [N][H] and start [H] float32")
    tokens = _host_i32(tokens)
    return _Embedding.apply(E, start, tokens.reshape(-1)).view(*tokens.shape, E.shape[1])


class _AttnCausal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, E, length, n_heads, n0, scale, p, seed, stream_id):
        if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape or any(t.dtype != torch.float32 for t in (q, k, v)):
            raise _lib.W2LInvalidArgument("attn_causal: q, k, v must be float32 [B][U][C]")
        B, U, Cc = q.shape
        if n_heads < 1 or Cc % n_heads:
            raise _lib.W2LInvalidArgument(f"attn_causal: C = {Cc} is no multiple of n_heads = {n_heads}")
        row = lambda t: t.stride(2) == 1 and t.stride(0) == U * t.stride(1) and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0
        if not (row(q) and row(k) and row(v) and q.stride(1) == k.stride(1) == v.stride(1)):   # else: thirds of one buffer, read in place
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if E is not None:
            E = E.contiguous()
            if E.dtype != torch.float32 or E.shape != (2 * n0 + 1, Cc // n_heads):
                raise _lib.W2LInvalidArgument(f"attn_causal: E must be float32 [2 n0 + 1 = {2 * n0 + 1}][d = {Cc // n_heads}]")
        ln = _host_i32(length)
        if ln.shape != (B,):
            raise _lib.W2LInvalidArgument("attn_causal: len must hold B lengths")
        d = _lib.AttnCausalDesc(B, n_heads, U, Cc // n_heads, q.stride(1), Cc, int(n0), float(scale), float(p), int(seed), int(stream_id))
        L = _lib.lib()
        out = torch.empty(B, U, Cc, device=q.device, dtype=torch.float32)
        lse = torch.empty(B, n_heads, U, device=q.device, dtype=torch.float32)
        nbytes = L.w2l_attn_causal_workspace_size(C.byref(d), 0)
        ws = _ws(nbytes, q.device)
        check(L.w2l_attn_causal_forward(C.byref(d), _p(q), _p(k), _p(v), _p(E), ln.ctypes.data, _p(out), _p(lse), _p(ws), nbytes, _s()),
              "attn_causal_forward")
        ctx.d, ctx.ln, ctx.has_E = d, ln, E is not None
        ctx.save_for_backward(q, k, v, E, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, E, lse = ctx.saved_tensors
        d, L = ctx.d, _lib.lib()
        B, U, Cc = dout.shape
        dout = dout.contiguous()
        # the gradients have the operands' row stride: thirds of one [B][U][3 C] buffer for an interleaved q | k | v, else three arrays
        if d.ld == 3 * Cc:
            g = torch.empty(B, U, 3 * Cc, device=dout.device, dtype=torch.float32)
            dq, dk, dv = g[..., :Cc], g[..., Cc:2 * Cc], g[..., 2 * Cc:]
        else:
            dq, dk, dv = (torch.empty(B, U, d.ld, device=dout.device, dtype=torch.float32)[..., :Cc] for _ in range(3))
        dE = torch.empty_like(E) if ctx.has_E else None
        nbytes = L.w2l_attn_causal_workspace_size(C.byref(d), 1)
        ws = _ws(nbytes, dout.device)
        check(L.w2l_attn_causal_backward(C.byref(d), _p(q), _p(k), _p(v), _p(E), ctx.ln.ctypes.data, _p(lse), _p(dout),
                                         _p(dq), _p(dk), _p(dv), _p(dE), _p(ws), nbytes, _s()), "attn_causal_backward")
        return dq, dk, dv, dE, None, None, None, None, None, None, None


def attn_causal(q, k, v, E, len, n_heads, n0, scale, p=0.0, seed=0, stream_id=0):
    """fused causal multi-head self-attention with a relative-position term (w2l_attn_causal_*): q, k, v [B][U][C] -- the
    thirds of one [B][U][3 C] buffer are read in place --, head h in columns h d .., E [2 n0 + 1][d] or None, len [B] on the host ->
    ctx [B][U][C] = dropout(softmax_j<=i(scale (q_i . k_j + q_i . E[j - i + n0]))) v, exactly 0 in the rows i >= len[b].  The dropout
    mask is ops.dropout_copy's over a dense [B][n_heads][U][U] array with the same (p, seed, stream_id).  Differentiable in q, k, v, E."""
    return _AttnCausal.apply(q, k, v, E, len, int(n_heads), int(n0), float(scale), float(p), int(seed), int(stream_id))


def _s2s_decode_operands(who, params, enc, key_len, keyvalue, beam, beam_token, max_len, nbest, eos, threshold, eos_score, attention_threshold,
                         temperature, lm_weight=0.0):
    """the checks that need no device, the descriptor and the operand pointers of the two decode calls"""
    E, start, rnn_p, W, bias = (t.contiguous() for t in params)
    if enc.dim() != 3 or E.dim() != 2 or any(t.dtype != torch.float32 for t in (enc, E, start, rnn_p, W, bias)):
        raise _lib.W2LInvalidArgument(f"{who}: enc [B][T][C], the embedding [N][H] and the other parameters must be float32")
    enc = enc.contiguous()
    (B, T, Cc), (N, H) = enc.shape, E.shape
    if Cc != (2 * H if keyvalue else H):
        raise _lib.W2LInvalidArgument(f"{who}: enc must have {'2 H' if keyvalue else 'H'} = {2 * H if keyvalue else H} columns, got {Cc}")
    if start.shape != (H,) or rnn_p.shape != (3 * H * (2 * H + 2),) or W.shape != (H, N) or bias.shape != (N,):
        raise _lib.W2LInvalidArgument(f"{who}: parameters must be E [N][H], start [H], the GRU's 3 H (2 H + 2) floats, W [H][N], bias [N]")
    kl = np.full(B, T, np.int32) if key_len is None else _host_i32(key_len)
    if kl.shape != (B,):
        raise _lib.W2LInvalidArgument(f"{who}: key_len must hold B lengths")
    d = _lib.S2sDecodeDesc(B, T, H, N, Cc, int(eos), int(beam), int(beam_token), int(max_len), int(nbest),
                           float("inf") if threshold is None else float(threshold), float(eos_score), float(temperature),
                           -1 if attention_threshold is None else int(attention_threshold), float(lm_weight))
    k = enc.data_ptr()
    return d, kl, (E, start, rnn_p, W, bias, enc), [_p(E), _p(start), _p(rnn_p), _p(W), _p(bias), k, k + 4 * H * int(keyvalue), kl.ctypes.data]


def s2s_decode(params, enc, key_len=None, keyvalue=False, *, eos, beam=1, beam_token=None, threshold=None, eos_score=0.0,
               attention_threshold=None, temperature=1.0, max_len=120, nbest=1, lm=None, lm_weight=0.0):
    """token beam search over the step-by-step decoder of a seq2seq model (w2l_s2s_decode).  params: the embedding
    [N][H], the start embedding [H], the GRU's flat parameter, the output weight [H][N] and bias [N]; enc [B][T][C] as
    ops.s2s_attention, key_len [B] on the host (None: T).  beam_token None: min(N, 64).  threshold None: no beam threshold;
    attention_threshold None: off.  -> (tokens [B][nbest][max_len] int32, -1 behind the end; lengths [B][nbest]; scores
    [B][nbest]) on the device; a hypothesis that does not exist has length 0 and score -inf.  beam 1 is greedy decoding.
    lm: an NGramLM over the N classes, fused into the search with lm_weight (w2l_s2s_decode_lm); a fourth result is then
    lm_scores [B][nbest], the hypotheses' unweighted LM scores."""
    N = params[0].shape[0]
    beam_token = min(N, 64) if beam_token is None else beam_token
    if lm is None and lm_weight:
        raise _lib.W2LInvalidArgument("s2s_decode: LM fusion (lm_weight) needs lm=")
    if lm is not None and lm.num_tokens != N:
        raise _lib.W2LInvalidArgument(f"s2s_decode: the LM has {lm.num_tokens} tokens, the model {N} classes")
    d, kl, keep, ptrs = _s2s_decode_operands("s2s_decode", params, enc, key_len, keyvalue, beam, beam_token, max_len, nbest, eos, threshold,
                                             eos_score, attention_threshold, temperature, lm_weight)
    L, dev = _lib.lib(), enc.device
    nbytes = (L.w2l_s2s_decode_workspace_size if lm is None else L.w2l_s2s_decode_lm_workspace_size)(C.byref(d))
    ws = _ws(nbytes, dev)
    tokens = torch.empty(d.B, max(d.nbest, 1), max(d.maxLen, 1), device=dev, dtype=torch.int32)
    lengths = torch.empty(d.B, max(d.nbest, 1), device=dev, dtype=torch.int32)
    scores = torch.empty(d.B, max(d.nbest, 1), device=dev, dtype=torch.float32)
    if lm is not None:
        lm_scores, blob = torch.empty_like(scores), lm.device_blob(dev)
        check(L.w2l_s2s_decode_lm(C.byref(d), *ptrs, _p(tokens), _p(lengths), _p(scores), _p(lm_scores), _p(ws), nbytes, _s(), _p(blob),
                                  int(lm.has_eos)), "s2s_decode")
        return tokens, lengths, scores, lm_scores
    check(L.w2l_s2s_decode(C.byref(d), *ptrs, _p(tokens), _p(lengths), _p(scores), _p(ws), nbytes, _s()), "s2s_decode")
    return tokens, lengths, scores


def s2s_decode_step(params, enc, parent, token, h_prev, key_len=None, keyvalue=False, *, beam, beam_token, temperature=1.0):
    """one decoder step for B x beam given rows (w2l_s2s_decode_step): parent, token [B][beam] on the host -- parent < 0
    is a dead row, of which nothing is written; else the slot of the same utterance whose row of h_prev [B][beam][H] is the previous
    state; token -1 is the start embedding with a zero state -> h, o [B][beam][H], peak [B][beam] (the first argmax of the
    attention), lse [B][beam] of z = (o W + bias) / temperature, and the min(beam_token, N) largest z of every row with their tokens,
    descending: cand_val, cand_tok [B][beam][beam_token]"""
    d, kl, keep, ptrs = _s2s_decode_operands("s2s_decode_step", params, enc, key_len, keyvalue, beam, beam_token, 1, 1, 0, None, 0.0, None,
                                             temperature)
    parent, token = _host_i32(parent), _host_i32(token)
    h_prev = None if h_prev is None else h_prev.contiguous()
    if parent.shape != (d.B, beam) or token.shape != parent.shape or (h_prev is not None and (h_prev.shape != (d.B, beam, d.H) or h_prev.dtype != torch.float32)):
        raise _lib.W2LInvalidArgument("s2s_decode_step: parent and token [B][beam] integers, h_prev [B][beam][H] float32")
    L, dev = _lib.lib(), enc.device
    nbytes = L.w2l_s2s_decode_workspace_size(C.byref(d))
    ws = _ws(nbytes, dev)
    f = lambda *s: torch.zeros(d.B, beam, *s, device=dev, dtype=torch.float32)
    i = lambda *s: torch.zeros(d.B, beam, *s, device=dev, dtype=torch.int32)
    h, o, peak, lse, cv, ct = f(d.H), f(d.H), i(), f(), f(beam_token), i(beam_token)
    check(L.w2l_s2s_decode_step(C.byref(d), *ptrs, parent.ctypes.data, token.ctypes.data, _p(h_prev), _p(h), _p(o), _p(peak), _p(lse), _p(cv), _p(ct),
                                _p(ws), nbytes, _s()), "s2s_decode_step")
    return h, o, peak, lse, cv, ct


def _ln_scratch(groups, inner):
    return int(_lib.lib().w2l_layernorm_scratch_doubles(groups, inner))


def residual_layernorm_forward(a, x, gamma_beta, groups, eps=1e-5, p=0.0, seed=0, stream_id=0):
    """returns (y, r, mean_rstd); `a` is dropped in place when p > 0"""
    inner = a.numel() // groups
    r = torch.empty_like(a)
    y = torch.empty_like(a)
    stats = torch.empty(_ln_scratch(groups, inner), device=a.device, dtype=torch.float64)
    mr = torch.empty(2 * groups, device=a.device, dtype=torch.float32)
    check(_lib.lib().w2l_residual_layernorm_forward(groups, inner, _p(a), _p(x), _p(r), _p(y), _p(gamma_beta), eps,
                                                    p, seed, stream_id, _p(stats), _p(mr), _s()), "res_ln_fwd")
    return y, r, mr


def layernorm_backward(r, dy, gamma_beta, mean_rstd, groups, mask_src=None, mask_scale=1.0):
    inner = r.numel() // groups
    dr = torch.empty_like(r)
    dgb = torch.empty(2, device=r.device, dtype=torch.float32)
    dmask = torch.empty_like(r) if mask_src is not None else None
    sums = torch.empty(_ln_scratch(groups, inner), device=r.device, dtype=torch.float64)
    check(_lib.lib().w2l_layernorm_backward(groups, inner, _p(r), _p(dy), _p(gamma_beta), _p(mean_rstd), _p(dr),
                                            _p(dgb), _p(mask_src), _p(dmask), mask_scale, _p(sums), _s()), "ln_bwd")
    return dr, dgb, dmask


def linear_forward_dropout(x, w, bias, relu, p, seed, stream_id):
    M, K = x.shape
    N = w.shape[1]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_linear_forward_dropout(M, K, N, _p(x), _p(w), _p(bias), _p(y), int(relu), p, seed, stream_id, _s()), "linear_forward_dropout")
    return y


def linear_forward_dropout_add(x, w, bias, add, relu, p, seed, stream_id):
    M, K = x.shape
    N = w.shape[1]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_linear_forward_dropout_add(M, K, N, _p(x), _p(w), _p(bias), _p(add), _p(y), int(relu), p, seed, stream_id, _s()),
          "linear_forward_dropout_add")
    return y


def linear_backward_data_add(dy, w, add):
    M, N = dy.shape
    K = w.shape[0]
    dx = torch.empty(M, K, device=dy.device, dtype=torch.float32)
    check(_lib.lib().w2l_linear_backward_data_add(M, K, N, _p(dy), _p(w), _p(add), _p(dx), _s()), "linear_bwd_data_add")
    return dx


def dropout_copy(x, p, seed, stream_id):
    y = torch.empty_like(x)
    check(_lib.lib().w2l_dropout_copy(_p(y), _p(x), x.numel(), p, seed, stream_id, _s()),
          "dropout_copy")
    return y


def dropout_(x, p, seed, stream_id):
    check(_lib.lib().w2l_dropout_inplace(_p(x), x.numel(), p, seed, stream_id, _s()), "dropout")
    return x


def transpose(x):
    """[G][R][C] -> [G][C][R]"""
    G, R, Cc = x.shape
    out = torch.empty(G, Cc, R, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_transpose(_p(x), _p(out), G, R, Cc, _s()), "transpose")
    return out


def glu_forward(x):
    M, two = x.shape
    y = torch.empty(M, two // 2, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_glu_forward(_p(x), _p(y), M, two // 2, _s()), "glu_fwd")
    return y


def glu_backward(x, dy):
    M, two = x.shape
    dx = torch.empty_like(x)
    check(_lib.lib().w2l_glu_backward(_p(x), _p(dy), _p(dx), M, two // 2, _s()), "glu_bwd")
    return dx


def sgd_step_(p, g, v, lr, momentum, grad_scale=1.0, max_grad_norm=0.0):
    L = _lib.lib()
    ss = torch.zeros(1, device=p.device, dtype=torch.float64)
    if max_grad_norm > 0:
        check(L.w2l_sumsq(_p(g), g.numel(), _p(ss), 1, _s()), "sumsq")
    check(L.w2l_sgd_step(_p(p), _p(g), _p(v), p.numel(), lr, momentum, grad_scale, max_grad_norm, _p(ss), _s()), "sgd")


def ema_update(ema, p, decay):
    """w2l_ema_update, in place: ema = decay * ema + (1 - decay) * p over two flat float32 CUDA tensors of one size (any float
    alignment; views into a parameter arena are fine).  slimIPL's averaged teacher network, one launch."""
    if not (torch.is_tensor(ema) and torch.is_tensor(p) and ema.is_cuda and p.is_cuda and ema.dtype == torch.float32
            and p.dtype == torch.float32 and ema.is_contiguous() and p.is_contiguous() and ema.numel() == p.numel()):
        raise _lib.W2LInvalidArgument("ema_update: two contiguous float32 CUDA tensors of the same size")
    check(_lib.lib().w2l_ema_update(_p(ema), _p(p), ema.numel(), float(decay), _s()), "ema_update")
    return ema


def bf16_convert(x, rows_image=True, transposed_image=False):
    """w2l_bf16_convert: x [rows][cols] fp32 -> (rowMajor [rows][colsP], transposed [cols][rowsP]) bf16 images, zero-padded to
    the next multiple of 64 (None for an image that was not asked for).  The images are torch.bfloat16 tensors."""
    x = x.contiguous()
    rows, cols = x.shape
    colsP, rowsP = (cols + 63) // 64 * 64, (rows + 63) // 64 * 64
    rm = torch.empty(rows, colsP, dtype=torch.bfloat16, device=x.device) if rows_image else None
    tr = torch.empty(cols, rowsP, dtype=torch.bfloat16, device=x.device) if transposed_image else None
    _lib.check(_lib.lib().w2l_bf16_convert(_p(x), rows, cols, cols, _p(rm) if rm is not None else None, colsP,
                                           _p(tr) if tr is not None else None, rowsP, _s()), "bf16_convert")
    return rm, tr


def bf16_convert_dropout(x, p, seed, stream_id, rows_image=True, transposed_image=True):
    """w2l_bf16_convert_dropout: the bf16 images of dropout(x) (mask of dropout_copy(p, seed, stream_id)) in one pass over x"""
    x = x.contiguous()
    rows, cols = x.shape
    colsP, rowsP = (cols + 63) // 64 * 64, (rows + 63) // 64 * 64
    rm = torch.empty(rows, colsP, dtype=torch.bfloat16, device=x.device) if rows_image else None
    tr = torch.empty(cols, rowsP, dtype=torch.bfloat16, device=x.device) if transposed_image else None
    _lib.check(_lib.lib().w2l_bf16_convert_dropout(_p(x), rows, cols, cols, _p(rm) if rm is not None else None, colsP,
                                                   _p(tr) if tr is not None else None, rowsP, p, seed, stream_id, _s()), "bf16_convert_dropout")
    return rm, tr


def gemm_bf16(A, B, K, bias=None, relu=False, mask=None, mask_scale=1.0, addend=None, out=None, accumulate=False,
              drop_p=0.0, drop_seed=0, drop_stream=0):
    """w2l_gemm_bf16: C[M][N] fp32 = A[M][>=K] . B[N][>=K]^T on bf16 images (rows zero from column K to the next multiple of 64)"""
    import ctypes as C
    M, N = A.shape[0], B.shape[0]
    c = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=A.device)
    e = _lib.GemmEpilogue()
    e.mask = _p(mask) if mask is not None else None
    e.maskScale = mask_scale
    e.addend = _p(addend) if addend is not None else None
    e.accumulate = int(accumulate)
    e.dropP = drop_p
    e.dropSeed, e.dropStream = drop_seed, drop_stream
    _lib.check(_lib.lib().w2l_gemm_bf16(M, N, K, _p(A), A.stride(0), _p(B), B.stride(0), _p(c), c.stride(0),
                                        _p(bias) if bias is not None else None, int(relu), C.byref(e), _s()), "gemm_bf16")
    return c


def gemm_split(A, B, a_kcontig=True, b_kcontig=False, bias=None, relu=False, mask=None, mask_scale=1.0, addend=None, out=None,
               accumulate=False, drop_p=0.0, drop_seed=0, drop_stream=0):
    """w2l_gemm_f32_split: C[M][N] fp32 = op(A) op(B) on the split-bf16 kernel (fp32 operands split into hi + lo bf16 in registers,
    three bf16 MFMA products per fp32 product, fp32 accumulation) whatever the process-wide switches say.  A is [M][K]
    (a_kcontig) or [K][M]; B is [N][K] (b_kcontig) or [K][N]; 2-d float32 CUDA tensors or views with unit inner stride.
    K >= 32.  The epilogue operands are w2l_gemm_bf16's."""
    import ctypes as C
    for t in (A, B):
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1):
            raise _lib.W2LInvalidArgument("gemm_split: 2-d float32 CUDA operands with unit inner stride")
    (M, K) = A.shape if a_kcontig else (A.shape[1], A.shape[0])
    (N, Kb) = B.shape if b_kcontig else (B.shape[1], B.shape[0])
    if K != Kb:
        raise _lib.W2LInvalidArgument(f"gemm_split: reduction lengths differ ({K} and {Kb})")
    c = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=A.device)
    e = _lib.GemmEpilogue()
    e.mask = _p(mask) if mask is not None else None
    e.maskScale = mask_scale
    e.addend = _p(addend) if addend is not None else None
    e.accumulate = int(accumulate)
    e.dropP = drop_p
    e.dropSeed, e.dropStream = drop_seed, drop_stream
    _lib.check(_lib.lib().w2l_gemm_f32_split(M, N, K, _p(A), A.stride(0), int(a_kcontig), _p(B), B.stride(0), int(b_kcontig), _p(c),
                                             c.stride(0), _p(bias) if bias is not None else None, int(relu), C.byref(e), _s()), "gemm_split")
    return c


def gemm_bf16_images(A, B, K, bias=None, relu=False, keep_f32=False, rows_image=True, transposed_image=True, mask_image=None,
                     mask_scale=1.0, addend=None, drop_p=0.0, drop_seed=0, drop_stream=0):
    """w2l_gemm_bf16_images: the product's result as bf16 images (zero-padded to multiples of 64 here, the caller's job in the ABI)
    instead of / beside the fp32 C; mask_image: a bf16 row-major image as the mask operand.  Returns (C or None, rows, transposed)."""
    import ctypes as C
    M, N = A.shape[0], B.shape[0]
    colsP, rowsP = (N + 63) // 64 * 64, (M + 63) // 64 * 64
    c = torch.empty(M, N, dtype=torch.float32, device=A.device) if keep_f32 else None
    rm = torch.zeros(M, colsP, dtype=torch.bfloat16, device=A.device) if rows_image else None
    tr = torch.zeros(N, rowsP, dtype=torch.bfloat16, device=A.device) if transposed_image else None
    e = _lib.GemmEpilogue()
    e.mask = None; e.maskScale = 1.0
    e.addend = _p(addend) if addend is not None else None
    e.accumulate = 0
    e.dropP = drop_p
    e.dropSeed, e.dropStream = drop_seed, drop_stream
    k = _lib.Bf16ImageSink()
    k.rowMajor = _p(rm) if rm is not None else None; k.ldRows = colsP
    k.transposed = _p(tr) if tr is not None else None; k.ldTrans = rowsP
    _lib.check(_lib.lib().w2l_gemm_bf16_images(M, N, K, _p(A), A.stride(0), _p(B), B.stride(0), _p(c) if c is not None else None, N,
                                               _p(bias) if bias is not None else None, int(relu), C.byref(e),
                                               C.byref(k) if (rm is not None or tr is not None) else None,
                                               _p(mask_image) if mask_image is not None else None,
                                               mask_image.stride(0) if mask_image is not None else 0, mask_scale, _s()), "gemm_bf16_images")
    return c, rm, tr


def gemm_bf16_ex(A, B, M, N, K, a_kmajor=False, b_kmajor=False, bias=None, relu=False):
    """w2l_gemm_bf16_ex: C[M][N] fp32 = op(A) op(B)^T with k-MAJOR operands read in place: a_kmajor -> A is [K][>= M],
    b_kmajor -> B is [K][>= N] (row strides multiples of 8 elements); otherwise as gemm_bf16"""
    c = torch.empty(M, N, dtype=torch.float32, device=A.device)
    _lib.check(_lib.lib().w2l_gemm_bf16_ex(M, N, K, _p(A), A.stride(0), int(a_kmajor), _p(B), B.stride(0), int(b_kmajor), _p(c), c.stride(0),
                                           _p(bias) if bias is not None else None, int(relu), None, _s()), "gemm_bf16_ex")
    return c


def gemm_bf16_grouped(As, Bs, K, biases=None):
    """w2l_gemm_bf16_grouped: [C_g = A_g . B_g^T (+ bias_g)] for up to 4 problems of one shape in one launch"""
    import ctypes as C
    n = len(As)
    M, N = As[0].shape[0], Bs[0].shape[0]
    outs = [torch.empty(M, N, dtype=torch.float32, device=As[0].device) for _ in range(n)]
    arr = lambda ts: (C.c_void_p * n)(*[(_p(t) if t is not None else None) for t in ts])
    _lib.check(_lib.lib().w2l_gemm_bf16_grouped(n, M, N, K, arr(As), As[0].stride(0), arr(Bs), Bs[0].stride(0), arr(outs), N,
                                                arr(biases) if biases is not None else None, _s()), "gemm_bf16_grouped")
    return outs


def tds_conv_bf16(x, w, bias, padl, padr, relu=False, stride=1):
    """the TDS / sub-sampling convolution on bf16-rounded operands (w2l_tds_conv_bf16_*): x [B][T][H][Cin], w [kw][Cin][Cout] ->
    y [B][To][H][Cout]; None when the geometry has no bf16 kernel"""
    import ctypes as C
    d = conv_desc(x, w, stride, padl, padr)
    n = _lib.lib().w2l_tds_conv_bf16_image_elems(C.byref(d))
    if not n:
        return None
    imgs = torch.empty(2, n, dtype=torch.bfloat16, device=x.device)
    check(_lib.lib().w2l_tds_conv_bf16_prepare(C.byref(d), _p(w), _p(imgs[0]), _p(imgs[1]), _s()), "tds_conv_bf16_prepare")
    To = _lib.lib().w2l_conv_out_len(d.T, d.kw, stride, padl, padr)
    y = torch.empty(d.B, To, d.H, d.Cout, device=x.device, dtype=torch.float32)
    check(_lib.lib().w2l_tds_conv_bf16_forward(C.byref(d), _p(x), _p(imgs[0]), _p(bias), _p(y), int(relu), _s()), "tds_conv_bf16_forward")
    return y, imgs, d


def tds_conv_bf16_backward(x, dy, imgs, d, add=None, with_bias=False):
    """(dx, dw[, db]) of the same convolution: dx = add + conv^T(dy), dw = x (*) dy, both on bf16-rounded operands; with_bias: the
    bias gradient (column sums of the rounded dy) from the same launch"""
    import ctypes as C
    dx = torch.empty_like(x)
    check(_lib.lib().w2l_tds_conv_bf16_backward_data(C.byref(d), _p(dy), _p(imgs[1]), _p(add), _p(dx), _s()), "tds_conv_bf16_backward_data")
    dw = torch.empty(d.kw, d.Cin, d.Cout, dtype=torch.float32, device=x.device)
    if with_bias:
        db = torch.empty(d.Cout, dtype=torch.float32, device=x.device)
        check(_lib.lib().w2l_tds_conv_bf16_backward_filter_bias(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _s()), "tds_conv_bf16_backward_filter_bias")
        return dx, dw, db
    check(_lib.lib().w2l_tds_conv_bf16_backward_filter(C.byref(d), _p(x), _p(dy), _p(dw), _s()), "tds_conv_bf16_backward_filter")
    return dx, dw


def conv_bf16(x, w, bias, padl, padr, relu=False, stride=1):
    """the wide time convolution at H == 1 on bf16-rounded operands (w2l_conv_bf16_*): x [B][T][1][Cin], w [kw][Cin][Cout] ->
    (y [B][To][1][Cout], (weight images, scratch), descriptor); None when the library has no kernel for the geometry"""
    import ctypes as C
    d = conv_desc(x, w, stride, padl, padr)
    L = _lib.lib()
    n = L.w2l_conv_bf16_image_elems(C.byref(d))
    if not n:
        return None
    imgs = torch.empty(2, n, dtype=torch.bfloat16, device=x.device)
    scratch = torch.empty(L.w2l_conv_bf16_scratch_elems(C.byref(d)), dtype=torch.bfloat16, device=x.device)
    check(L.w2l_conv_bf16_prepare(C.byref(d), _p(w), _p(imgs[0]), _p(imgs[1]), _s()), "conv_bf16_prepare")
    To = L.w2l_conv_out_len(d.T, d.kw, stride, padl, padr)
    y = torch.empty(d.B, To, d.H, d.Cout, device=x.device, dtype=torch.float32)
    check(L.w2l_conv_bf16_forward(C.byref(d), _p(x), _p(imgs[0]), _p(bias), _p(y), int(relu), _p(scratch), _s()), "conv_bf16_forward")
    return y, (imgs, scratch), d


def conv_bf16_backward(x, dy, imgs, d, add=None, with_bias=False):
    """(dx, dw[, db]) of the same convolution (imgs: the pair conv_bf16 returned): dx = add + conv^T(dy), dw = x (*) dy on the
    bf16-rounded operands; with_bias: the bias gradient, the column sums of the rounded dy"""
    import ctypes as C
    imgs, scratch = imgs
    L = _lib.lib()
    dx = torch.empty_like(x)
    check(L.w2l_conv_bf16_backward_data(C.byref(d), _p(dy), _p(imgs[1]), _p(add), _p(dx), _p(scratch), _s()), "conv_bf16_backward_data")
    dw = torch.empty(d.kw, d.Cin, d.Cout, dtype=torch.float32, device=x.device)
    db = torch.empty(d.Cout, dtype=torch.float32, device=x.device) if with_bias else None
    check(L.w2l_conv_bf16_backward_filter_bias(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(scratch), _s()), "conv_bf16_backward_filter_bias")
    return (dx, dw, db) if with_bias else (dx, dw)

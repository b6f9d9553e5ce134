"""The bottleneck window attention of ACVNet_DDIM's hourglasses in training on HIP kernels (csrc/window_attn.hip forward,
csrc/window_attn_bwd.hip backward).

``window_attention_train(x, qkv_w, qkv_b, proj_w, proj_b, heads)`` is attention_block.forward
(SceneFlow/models/submodule.py:398-429): multi-head self-attention inside 4 x 4 x 4 windows of x [B,128,D,H,W], H and W
zero-padded up to whole windows, followed by the 1x1x1 convolution ``final1x1``, as one ``torch.autograd.Function``:
  * forward: ``dv_window_attn3d_f32``, the eval path's kernel (the bits of ``submodule.window_attention``);
  * backward: ``dv_window_attn3d_bwd_f32`` -- one block per window recomputes the probabilities with the forward's
    arithmetic and writes the input gradient once; the two weight gradients are split-K GEMMs over the tokens and the two
    bias gradients fixed-order sums.  Only ``x`` and the four parameters are saved: not the padded copy, the permuted
    copies, q, k, v, the [B, windows, 16, 64, 64] logits and probabilities or the merged heads.  No atomics: the same bits on
    every launch.  A gradient that is not needed is not computed.
There is no double backward.  ``DV_TRAIN_ATTN=torch`` routes the function to the PyTorch statement (A/B runs, tests).
CPU tensors raise, as everywhere on the hot path."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _env, _lib, train3d


route = functools.partial(_env.route, "DV_TRAIN_ATTN")


def _statement(x, qkv_w, qkv_b, proj_w, proj_b, heads, block: int = 4):
    """The PyTorch statement.  The reference's padding mask (-1000 between a padded and an unpadded token) only takes
    effect when H AND W are both padded: with one of them whole, its ``mask[:, -0:]`` slice marks every token (the eval
    kernel, csrc/window_attn.hip, does the same)."""
    b, c, d, h0, w0 = x.shape
    ph, pw = (-h0) % block, (-w0) % block
    xp = F.pad(x, (0, pw, 0, ph))
    h, w = h0 + ph, w0 + pw
    nd, nh, nw = d // block, h // block, w // block
    nwin, ntok = nd * nh * nw, block ** 3
    ch = c // heads
    # tokens of one window contiguous: [B, windows, tokens, C], token = (z, y, x) inside the window
    tok = xp.reshape(b, c, nd, block, nh, block, nw, block).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(b, nwin, ntok, c)
    qkv = F.linear(tok, qkv_w, qkv_b).reshape(b, nwin, ntok, 3, heads, ch)
    q, k, v = qkv.permute(3, 0, 1, 4, 2, 5).unbind(0)                  # [B, windows, heads, tokens, ch]
    logits = (q @ k.transpose(-2, -1)) * ch ** -0.5
    if ph and pw:
        rows = torch.arange(h, device=x.device).view(nh, 1, block, 1) >= h0
        cols = torch.arange(w, device=x.device).view(1, nw, 1, block) >= w0
        padded = (rows | cols).reshape(nh * nw, 1, block * block)    # [h*w windows, 1, in-plane]
        padded = padded.expand(nh * nw, block, block * block).reshape(nh * nw, ntok)      # depth repeats the plane
        padded = padded.repeat(nd, 1)                                                      # [windows, tokens]
        bias = torch.zeros((nwin, ntok, ntok), dtype=logits.dtype, device=x.device)
        bias = bias.masked_fill(padded.unsqueeze(2) != padded.unsqueeze(1), -1000.0)
        logits = logits + bias.unsqueeze(1)
    y = torch.softmax(logits, dim=-1) @ v                               # [B, windows, heads, tokens, ch]
    y = y.reshape(b, nd, nh, nw, heads, block, block, block, ch).permute(0, 4, 8, 1, 5, 2, 6, 3, 7)
    y = y.reshape(b, c, d, h, w)[:, :, :, :h0, :w0]
    return train3d.conv3d(y, proj_w.reshape(c, c, 1, 1, 1), proj_b, stride=1)


class WindowAttentionFn(torch.autograd.Function):
    """x [B,128,D,H,W], qkv_w [384,128], qkv_b [384], proj_w [128,128], proj_b [128]; saves its five inputs only."""

    @staticmethod
    def forward(ctx, x, qkv_w, qkv_b, proj_w, proj_b, heads):
        x, qkv_w, qkv_b, proj_w, proj_b = (t.contiguous() for t in (x, qkv_w, qkv_b, proj_w, proj_b))
        b, c, d, h, w = x.shape
        out = torch.empty_like(x)
        _lib.launch("dv_window_attn3d_f32", x.device, x.data_ptr(), qkv_w.data_ptr(), qkv_b.data_ptr(), proj_w.data_ptr(),
                    proj_b.data_ptr(), out.data_ptr(), b, c, d, h, w, heads)
        ctx.save_for_backward(x, qkv_w, qkv_b, proj_w, proj_b)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, qkv_w, qkv_b, proj_w, proj_b = ctx.saved_tensors
        want = ctx.needs_input_grad[:5]
        if not any(want):
            return None, None, None, None, None, None
        _lib.check_f32(dout, "grad_output")
        dout = dout.contiguous()
        b, c, d, h, w = x.shape
        grads = [torch.empty_like(t) if wanted else None for t, wanted in zip((x, qkv_w, qkv_b, proj_w, proj_b), want)]
        ws = None
        if want[1] or want[2] or want[3]:
            ws = _lib.workspace("dv_window_attn3d_bwd_workspace_floats", x.device, b, c, d, h, w, ctx.heads)
        _lib.launch("dv_window_attn3d_bwd_f32", x.device, x.data_ptr(), qkv_w.data_ptr(), qkv_b.data_ptr(), proj_w.data_ptr(),
                    dout.data_ptr(), *(_lib.ptr(g) for g in grads), _lib.ptr(ws), b, c, d, h, w, ctx.heads)
        return (*grads, None)


def window_attention_train(x: torch.Tensor, qkv_w: torch.Tensor, qkv_b: torch.Tensor, proj_w: torch.Tensor,
                           proj_b: torch.Tensor, heads: int = 16) -> torch.Tensor:
    """attention_block.forward for x [B,C,D,H,W] with ``qkv_3d.weight`` [3C,C], ``qkv_3d.bias`` [3C], ``final1x1.weight``
    ([C,C] or [C,C,1,1,1]) and ``final1x1.bias`` [C], differentiable in all five.  Returns a fresh tensor."""
    r = route()
    for name, t in (("x", x), ("qkv_w", qkv_w), ("qkv_b", qkv_b), ("proj_w", proj_w), ("proj_b", proj_b)):
        _lib.check_f32(t, name)
    if x.dim() != 5:
        raise RuntimeError(f"x must be [B,C,D,H,W], got {tuple(x.shape)}")
    c = x.shape[1]
    if tuple(qkv_w.shape) != (3 * c, c) or tuple(qkv_b.shape) != (3 * c,):
        raise RuntimeError(f"qkv_w and qkv_b must be {(3 * c, c)} and {(3 * c,)}, got {tuple(qkv_w.shape)} and "
                           f"{tuple(qkv_b.shape)}")
    if proj_w.numel() != c * c or tuple(proj_w.shape[:2]) != (c, c) or tuple(proj_b.shape) != (c,):
        raise RuntimeError(f"proj_w and proj_b must be {(c, c)} and {(c,)}, got {tuple(proj_w.shape)} and "
                           f"{tuple(proj_b.shape)}")
    if x.numel() == 0:
        raise RuntimeError(f"x is empty: {tuple(x.shape)}")
    heads = int(heads)
    if r == "torch":
        return _statement(x, qkv_w, qkv_b, proj_w, proj_b, heads)
    return WindowAttentionFn.apply(x, qkv_w, qkv_b, proj_w.reshape(c, c), proj_b, heads)

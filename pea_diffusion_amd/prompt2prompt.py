"""Prompt-to-Prompt editing (Hertz et al., 2022): keep the picture, change one word.

A batch holds N prompts denoised from the SAME initial latents.  One of them is the source; an edited prompt b takes part of
its attention from its source s = src[b].  In every cross-attention layer, per head, with L context rows

    P0 = softmax(scale Q[s] K[s]^T)      the source's probabilities at the same query positions
    P1 = softmax(scale Q[b] K[b]^T)      its own
    A[q, j] = c[b, j] * sum_k P0[q, k] * Mt[b, j, k]  +  d[b, j] * P1[q, j],       O[b] = A V[b]

(`ops.attention_fwd_edit`, `HipUNet.set_prompt_edit`).  The per-key factors c and d fold the whole controller chain of the paper's
code into two numbers per key and step.  With w the cross-replace weight of key j at this step, a the refinement alpha of key j
(1 where the target token has a source token, 0 where it is new) and e the equalizer of key j, applying the controllers one after
another gives

    word swap          replaced = P0 M                 out = w e replaced + (1 - w) P1          c = w e,    d = 1 - w
    refinement         replaced = a P0[g] + (1 - a) P1 out = w e replaced + (1 - w) P1          c = w a e,  d = 1 - w + w (1 - a) e
    re-weighting       replaced = P0                   out = w e replaced + (1 - w) P1          c = w e,    d = 1 - w,  Mt = identity

(d of the refinement is 1 - w a wherever e = 1 or a = 1, the usual case: the equalizer's factor on a NEW token scales that
token's own attention, as it does in the original.)  Once the window of every key has ended c = 0 and d = 1 everywhere and the
layer runs its plain launch.  In the self-attention layers with at most `self_max_tokens` queries, while step < self_until, an
edited sample attends with its source's probabilities: O[b] = softmax(scale Q[s] K[s]^T) V[b].

Everything here is host-side and float64; token ids come from the caller (no tokenizer is used).  With classifier-free guidance
the batch is [uncond x N | cond x N] and only the conditional half is ever edited, as in the original."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from ._lib import PeaError

F64 = torch.float64


def replace_mapper(L: int, spans) -> torch.Tensor:
    """Word swap -> M fp64 [L, L], row = source key, column = target key (Mt of the kernel is its transpose).
    spans: [((s0, s1), (t0, t1)), ...], source tokens s0 .. s1 - 1 become target tokens t0 .. t1 - 1, in ascending order.  One to
    one where the lengths agree; an averaging block of 1 / (t1 - t0) where they do not (every source token of the span feeds every
    target token of it); identity elsewhere, shifted by the length differences of the spans in front."""
    M = torch.zeros(L, L, dtype=F64)
    spans = sorted(((int(a), int(b)), (int(c), int(d))) for (a, b), (c, d) in spans)
    i = j = 0
    k = 0
    while i < L and j < L:
        if k < len(spans) and spans[k][0][0] == i:
            (s0, s1), (t0, t1) = spans[k]
            if not (s0 < s1 <= L and t0 < t1 <= L and t0 == j):
                raise PeaError(f"replace_mapper: span {spans[k]} does not fit (source position {i} is target position {j}, L={L})")
            if s1 - s0 == t1 - t0:
                for n in range(s1 - s0):
                    M[s0 + n, t0 + n] = 1.0
            else:
                M[s0:s1, t0:t1] = 1.0 / (t1 - t0)
            i, j, k = s1, t1, k + 1
        else:
            if k < len(spans) and spans[k][0][0] < i:
                raise PeaError(f"replace_mapper: spans overlap at source position {i}")
            M[i, j] = 1.0
            i, j = i + 1, j + 1
    if k < len(spans):
        raise PeaError(f"replace_mapper: span {spans[k]} lies outside the context of {L} rows")
    return M


def refine_mapper(src_ids: Sequence[int], tgt_ids: Sequence[int], L: Optional[int] = None):
    """Prompt refinement -> (gather int64 [L], alphas fp64 [L]): gather[j] is the source key of target key j, or -1 where target
    token j is new (alpha 0).  A global alignment (Needleman-Wunsch) of the two token-id lists with match +1, mismatch -1, gap -1;
    aligned but different tokens count as mapped (alpha 1).  Ties prefer a gap in the source, then a gap in the target, then the
    diagonal, as the original does.  Positions at and past len(tgt_ids) map to themselves."""
    x, y = [int(t) for t in src_ids], [int(t) for t in tgt_ids]
    L = max(len(x), len(y)) if L is None else int(L)
    if len(x) > L or len(y) > L:
        raise PeaError(f"refine_mapper: {len(x)} / {len(y)} tokens in a context of {L} rows")
    n, m = len(x), len(y)
    score = [[0] * (m + 1) for _ in range(n + 1)]
    back = [[0] * (m + 1) for _ in range(n + 1)]          # 1: from the left (new target token), 2: from above, 3: diagonal
    for j in range(1, m + 1):
        score[0][j], back[0][j] = -j, 1
    for i in range(1, n + 1):
        score[i][0], back[i][0] = -i, 2
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            left, up = score[i][j - 1] - 1, score[i - 1][j] - 1
            diag = score[i - 1][j - 1] + (1 if x[i - 1] == y[j - 1] else -1)
            best = max(left, up, diag)
            score[i][j] = best
            back[i][j] = 1 if best == left else 2 if best == up else 3
    gather = torch.arange(L, dtype=torch.int64)
    alphas = torch.ones(L, dtype=F64)
    i, j = n, m
    while i > 0 or j > 0:
        if back[i][j] == 3:
            i, j = i - 1, j - 1
            gather[j] = i
        elif back[i][j] == 1:
            j -= 1
            gather[j] = -1
            alphas[j] = 0.0
        else:
            i -= 1
    return gather, alphas


def gather_mapper(gather: torch.Tensor) -> torch.Tensor:
    """the gather of `refine_mapper` as M fp64 [L, L] (row = source key, column = target key): one-hot columns, a zero column
    where the target token is new"""
    L = gather.numel()
    M = torch.zeros(L, L, dtype=F64)
    for j, g in enumerate(gather.tolist()):
        if g >= 0:
            if g >= L:
                raise PeaError(f"gather_mapper: source index {g} outside the context of {L} rows")
            M[g, j] = 1.0
    return M


def equalizer(L: int, values=None) -> torch.Tensor:
    """Attention re-weighting -> fp64 [L]: 1 everywhere, `values[index]` at the given keys (any finite value; negative flips)."""
    e = torch.ones(L, dtype=F64)
    for k, v in (values or {}).items():
        if not 0 <= int(k) < L or not math.isfinite(float(v)):
            raise PeaError(f"equalizer: key {k} -> {v} (0 <= key < {L}, a finite value)")
        e[int(k)] = float(v)
    return e


def _window(T, bounds):
    lo, hi = (0.0, float(bounds)) if not isinstance(bounds, (tuple, list)) else (float(bounds[0]), float(bounds[1]))
    if not (0.0 <= lo <= hi <= 1.0):
        raise PeaError(f"cross_schedule: window {bounds} (fractions of the steps, 0 <= start <= end <= 1)")
    return int(math.floor(lo * T + 1e-9)), int(math.floor(hi * T + 1e-9))


def cross_schedule(T: int, L: int, cross_replace_steps, per_token=None) -> torch.Tensor:
    """-> w fp64 [T, L]: 1 while the source's attention is injected into key j, 0 afterwards.  cross_replace_steps: a fraction
    f of the steps (steps 0 .. floor(f T) - 1) or (start, end) fractions; per_token {key index: fraction or pair} overrides it
    for single keys."""
    if T < 1 or L < 1:
        raise PeaError(f"cross_schedule: T={T}, L={L}")
    w = torch.zeros(T, L, dtype=F64)
    lo, hi = _window(T, cross_replace_steps)
    w[lo:hi] = 1.0
    for k, b in (per_token or {}).items():
        if not 0 <= int(k) < L:
            raise PeaError(f"cross_schedule: key {k} outside the context of {L} rows")
        lo, hi = _window(T, b)
        w[:, int(k)] = 0.0
        w[lo:hi, int(k)] = 1.0
    return w


def fold(w: torch.Tensor, alphas=None, eq=None):
    """the controller chain as two factors per key: w fp64 [T, L], alphas / eq fp64 [L] or None -> (c, d) fp64 [T, L]"""
    a = torch.ones_like(w[0]) if alphas is None else alphas.to(F64)
    e = torch.ones_like(w[0]) if eq is None else eq.to(F64)
    return w * a * e, 1.0 - w + w * (1.0 - a) * e


@dataclass
class PromptEdit:
    """The tables of one batch: src int64 [B] (negative: not edited), Mt fp64 [B, L, L] (row = target key, column = source key),
    cd fp64 [T, 2, B, L] (c then d for every step), the self-attention rule.  `cfg`: the batch is [uncond x N | cond x N]."""
    src: torch.Tensor
    Mt: torch.Tensor
    cd: torch.Tensor
    self_until: int
    self_max_tokens: int = 1024
    cfg: bool = False

    @property
    def T(self):
        return self.cd.shape[0]

    @staticmethod
    def compose(L: int, T: int, edits, cross_replace_steps=0.8, self_replace_steps=0.4, self_max_tokens: int = 1024,
                do_cfg: bool = False) -> "PromptEdit":
        """edits: one entry per prompt of the batch -- None for an unedited prompt (a source), or a dict with
        `source` (index of an unedited prompt), and optionally `mapper` (M of `replace_mapper`: word swap), `refine`
        ((gather, alphas) of `refine_mapper`: refinement; not together with `mapper`), `equalizer` (fp64 [L]: re-weighting, alone
        or after either), `cross_replace_steps` / `per_token` (this prompt's own window).  self_replace_steps: the fraction of
        the steps during which the self-attention rule applies.  do_cfg: lay the tables out for [uncond x N | cond x N]."""
        edits = list(edits)
        N = len(edits)
        if N < 1:
            raise PeaError("PromptEdit.compose: no prompts")
        src = torch.full((N,), -1, dtype=torch.int64)
        Mt = torch.eye(L, dtype=F64).repeat(N, 1, 1)
        cd = torch.zeros(T, 2, N, L, dtype=F64)
        cd[:, 1] = 1.0
        for b, ed in enumerate(edits):
            if ed is None:
                continue
            s = int(ed["source"])
            if not 0 <= s < N or edits[s] is not None:
                raise PeaError(f"PromptEdit.compose: prompt {b} names source {s}, which is not an unedited prompt of the {N}")
            if ed.get("mapper") is not None and ed.get("refine") is not None:
                raise PeaError(f"PromptEdit.compose: prompt {b} has both a word-swap mapper and a refinement")
            alphas = None
            if ed.get("mapper") is not None:
                M = torch.as_tensor(ed["mapper"]).to(F64)
            elif ed.get("refine") is not None:
                gather, alphas = ed["refine"]
                M = gather_mapper(torch.as_tensor(gather))
            else:
                M = torch.eye(L, dtype=F64)
            if tuple(M.shape) != (L, L):
                raise PeaError(f"PromptEdit.compose: mapper {tuple(M.shape)} of prompt {b}, expected ({L}, {L})")
            w = cross_schedule(T, L, ed.get("cross_replace_steps", cross_replace_steps), ed.get("per_token"))
            c, d = fold(w, alphas, ed.get("equalizer"))
            src[b], Mt[b] = s, M.t()
            cd[:, 0, b], cd[:, 1, b] = c, d
        self_until = _window(T, self_replace_steps)[1]
        pe = PromptEdit(src, Mt, cd, self_until, int(self_max_tokens))
        return pe.with_cfg() if do_cfg else pe

    def with_cfg(self) -> "PromptEdit":
        """the same edit for the classifier-free-guidance batch [uncond x N | cond x N]: the unconditional half is never edited"""
        if self.cfg:
            return self
        N, L = self.src.numel(), self.Mt.shape[-1]
        src = torch.cat([torch.full((N,), -1, dtype=torch.int64), torch.where(self.src >= 0, self.src + N, self.src)])
        Mt = torch.cat([torch.eye(L, dtype=F64).repeat(N, 1, 1), self.Mt])
        plain = torch.zeros(self.T, 2, N, L, dtype=F64)
        plain[:, 1] = 1.0
        return PromptEdit(src, Mt, torch.cat([plain, self.cd], 2), self.self_until, self.self_max_tokens, True)


def denoise_edit(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, edit: PromptEdit, num_inference_steps: int = 30,
                 guidance_scale: float = 7.5, callback=None, **kw):
    """`sampler.denoise` over the N prompts of `edit` from ONE initial latent: latents [1, C, h, w] (or already [N, ...]) are
    expanded to the N prompts, the edit is set at step 0 and advanced through denoise's `callback`, and cleared at the end.
    prompt_embeds / added_cond_kwargs are the batch's, laid out as denoise takes them ([uncond x N | cond x N] with guidance).
    edit.T must be num_inference_steps."""
    from .sampler import denoise
    do_cfg = guidance_scale > 1.0
    N = edit.src.numel() // (2 if edit.cfg else 1)
    if edit.T != num_inference_steps:
        raise PeaError(f"denoise_edit: the edit has tables for {edit.T} steps, the loop runs {num_inference_steps}")
    if latents.shape[0] == 1:
        latents = latents.expand(N, -1, -1, -1)
    if latents.shape[0] != N:
        raise PeaError(f"denoise_edit: {latents.shape[0]} latents for {N} prompts")
    unet.set_prompt_edit(edit, do_cfg=do_cfg)
    unet.set_prompt_edit_step(0)

    def advance(i, t, lat):
        if i + 1 < edit.T:
            unet.set_prompt_edit_step(i + 1)
        if callback is not None:
            callback(i, t, lat)

    try:
        return denoise(unet, scheduler, latents.contiguous(), prompt_embeds, added_cond_kwargs,
                       num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, callback=advance, **kw)
    finally:
        unet.clear_prompt_edit()

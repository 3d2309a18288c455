"""Shared by tests/test_gpu_backward_rows.py and tests/test_backward_rows_cpu.py (no test in here): fp64 references of every stage of the bf16
backbone backward, each fed with the engine's own inputs to that stage (teacher-forced), the comparators, and a CPU emulation of a whole
forward + backward that stands in the kernels' place where there is no GPU.

A `run` is what the GPU test captures from the engine (test_gpu_backward_rows._case) or what emulate_run() makes: a dict of fp64 CPU
tensors
    depth, B        ints
    fwd[i]          xhat1 (M,192), rstd1 (M), qkv (M,576), lse (B,3,197), attn_o, xhat2 (M,192), rstd2 (M), act, dact (M,768)
    bwd[i]          dx_in, dx_mid, dO, dx_out (M,192), dpre (M,768), dqkv (M,576)
    xhat_cls (B,192), rstd_cls (B), dfeat (B,192), grads {parameter name: gradient}, xgrad (B,3,224,224) or None
with M = B * 197.  The LAST block runs everything behind its attention on the class-token rows: its attn_o, xhat2, rstd2, act, dact, dx_in,
dx_mid, dO and dpre hold B rows, its lse is (B,3,1) (the class token's query); dqkv and dx_out hold every row.

Two references per dgrad stage, both fp64:
  R  the truth: the formula on the fp32 master weights, nothing rounded;
  E  the emulation: the same formula with its operands rounded to bf16 where the kernel rounds them.  The rounding points, read from
     csrc/vit.hip (vit_prepare_impl, vit_backward_impl), gemm.hip (EPI_MUL, EPI_BF16, EPI_LNBWD), mlp_fused.hip (KIND = 1 and FRONT),
     attention.hip (attn_bwd, attn_cls_bwd_kernel) and cls_tail.hip (cls_tail_bwd_kernel):
       * weight images: bf16(W) for fc2 and proj, bf16(W * gamma) (fp32 product) for fc1 and qkv; every dgrad GEMM sums bf16 x bf16 in fp32
       * A1  dpre = bf16(bf16(dx_in W2) * dact)                       the fc2 dgrad is staged in bf16 before the multiply by gelu'
       * A2  dx_mid = bf16(dx_in + LNbwd(bf16(dpre W1f); xhat2, rstd2))   the fc1 dgrad is staged in bf16; the LayerNorm backward and the
             residual sum are fp32.  In the last block dx_in is the fp32 final-norm backward of d_features, not its stored bf16 rows
       * A3  dO = bf16(dx_mid Wproj)
       * A4  delta = rowsum(dO * attn_o) and lse come from the forward's saved fields; P * 2^-3 = exp2(S c - lse - 3) and
             dS * 2^-3 = P * 2^-3 * (dO V^T - delta) are fp32 and rounded to bf16 as the operands of the dV, dK and dQ products (the factor
             2^-3 is exact); dqkv = bf16(...).  The last block's rank-one form (attn_cls_bwd_kernel) keeps P and dS in fp32
       * A5  dx_out = bf16(dx_mid + LNbwd(bf16(dqkv Wqkvf); xhat1, rstd1)); in the last block dx_mid is zero off the class-token rows
     The stage's own output rounding is not applied to E: the bounds carry it as half a bf16 ulp of the row.
Parameter gradients are sums of exact bf16 x bf16 products accumulated in fp32 (gemm.hip wgrad_kernel, wgrad_reduce_batch_kernel): their
reference is the fp64 sum of the engine's own buffers and their bound is derived, see grad_refs()."""
import math

import torch
import torch.nn.functional as F

from oracle import ref_cpu

ROWS, D, MLP, HEADS, HD = 197, 192, 768, 3, 64
EPS = 1e-6
REL = 2e-3                 # the relative term of the project's bounds for these epilogues (test_gpu_round3.py, test_gpu_block_bwd.py)
ULP = 2.0 ** -7            # one bf16 ulp of x is at most 2^-7 |x|
HALF_ULP = 2.0 ** -8
FLOOR = 2.0 ** -20         # a row's scale is at least this share of the tensor's largest element
U32 = 2.0 ** -23
GELU2_MAX = 0.80           # max |gelu''|
LSE_TOL = 1e-3
LOG2E = 1.0 / math.log(2.0)


def bf(t):
    """fp64 -> the nearest bf16 (through fp32, as the kernels' fp32 accumulators are rounded), back in fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def vit_sd(depth, seed, peaked=False):
    """init_vit_state weights; peaked: qkv weights at std 0.15 and LayerNorm gamma = 1 + N(0, 0.3) (test_gpu_token_rows._vit_sd)."""
    g = torch.Generator().manual_seed(seed)
    sd = ref_cpu.init_vit_state(depth, g)
    if peaked:
        for i in range(depth):
            b = f'blocks.{i}.'
            sd[b + 'attn.qkv.weight'] = torch.randn(576, 192, generator=g) * 0.15
            for n in ('norm1', 'norm2'):
                sd[b + n + '.weight'] = 1.0 + 0.3 * torch.randn(192, generator=g)
    return sd


def images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def loss_weights(B, seed):
    """w of the loss (features * w).sum(): d_features = w."""
    return torch.randn(B, D, generator=torch.Generator().manual_seed(seed))


def patches(x):
    """(B * 196, 768) patch rows in the patch weight's column order c * 256 + ky * 16 + kx."""
    return F.unfold(x.double(), 16, stride=16).transpose(1, 2).reshape(-1, 768)


def block_weights(sd, i):
    """fp64 masters, the truth's folds (W * gamma) and the engine's bf16 images of block i."""
    p = lambda n: sd[f'blocks.{i}.{n}']                      # noqa: E731
    w = {}
    for name, key, norm in (('fc1', 'mlp.fc1', 'norm2'), ('qkv', 'attn.qkv', 'norm1')):
        W, b, g, be = p(key + '.weight'), p(key + '.bias'), p(norm + '.weight'), p(norm + '.bias')
        w[name] = W.double()
        w[name + '_b'] = b.double()
        w[name + '_g'] = W.double() * g.double()
        w[name + '_f'] = (W * g).to(torch.bfloat16).double()                       # prep_weight_kernel: bf16(W[n][k] * gamma[k])
        w[name + '_bf'] = b.double() + W.double() @ be.double()                    # b + W beta (fp32 there; the difference is ~1e-8)
        w[name + '_gamma'], w[name + '_beta'] = g.double(), be.double()
    for name, key in (('fc2', 'mlp.fc2'), ('proj', 'attn.proj')):
        w[name] = p(key + '.weight').double()
        w[name + '_b'] = p(key + '.bias').double()
        w[name + '_f'] = p(key + '.weight').to(torch.bfloat16).double()
    return w


def ln(t):
    """LayerNorm without its affine, and 1 / sqrt(var + eps) (biased variance)."""
    var = t.var(dim=-1, unbiased=False, keepdim=True)
    return (t - t.mean(-1, keepdim=True)) * (var + EPS).rsqrt(), (var + EPS).rsqrt().squeeze(-1)


def ln_bwd(v, xhat, rstd):
    return rstd[:, None] * (v - v.mean(1, keepdim=True) - xhat * (v * xhat).mean(1, keepdim=True))


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def heads_of(qkv, B):
    """(M,576) -> q, k, v (B,3,197,64)."""
    return qkv.view(B, ROWS, 3, HEADS, HD).permute(2, 0, 3, 1, 4)


def rows_of(t, B):
    """(B,3,197,64) -> (M,192)."""
    return t.transpose(1, 2).reshape(B * ROWS, D)


def attention(qkv, B):
    """fp64 attention of qkv rows: the output before proj (M,192), the log2-sum-exp (B,3,197), every softmax row's largest probability."""
    q, k, v = heads_of(qkv, B)
    s = (q @ k.transpose(-2, -1)) * 0.125
    a = torch.softmax(s, dim=-1)
    return rows_of(a @ v, B), torch.logsumexp(s, dim=-1) * LOG2E, a.amax(-1).flatten()


def cls_to_full(t, B):
    """(B,w) class-token rows -> (M,w), zeros elsewhere."""
    full = torch.zeros(B, ROWS, t.shape[-1], dtype=t.dtype)
    full[:, 0] = t
    return full.view(B * ROWS, -1)


# ---- references of the dgrad stages ------------------------------------------------------------------------------------------------

class Stage:
    """One tensor of one block: got (the engine's), R, E (E: output not rounded), extra = the absolute per-row terms of the E bound beyond
    REL x the row's scale, kind 'E+R' (both comparators) or 'R' (the attention backward: against R only)."""

    def __init__(self, name, block, got, R, E, extra, kind='E+R'):
        self.name, self.block, self.got, self.R, self.E, self.extra, self.kind = name, block, got, R, E, extra, kind


def row_scale(ref):
    r = ref.reshape(ref.shape[0], -1).abs()
    return r.amax(1).clamp_min(FLOOR * float(r.max()))


def row_err(got, ref):
    return (got.reshape(ref.shape[0], -1) - ref.reshape(ref.shape[0], -1)).abs().amax(1)


def stage_ratios(st, got=None):
    """Per row: (error against E / its bound, error against R / its bound, the worst per-row distance of E from R in units of the row's
    scale).  The E ratio is None for kind 'R'.  A row that is not finite gives NaN."""
    got = st.got if got is None else got
    sE, sR = row_scale(st.E), row_scale(st.R)
    dist = float((row_err(st.E, st.R) / sR).max())
    if st.kind == 'R':
        # no project bound of its own: twice the emulation's distance from the truth plus one bf16 ulp of the output row
        return None, row_err(got, st.R) / (2.0 * dist * sR + ULP * sR), dist
    bE = REL * sE + st.extra
    # (2 x: fp32 against fp64 accumulation and summation order on top of the roundings E shares with the kernel)
    return row_err(got, st.E) / bE, row_err(got, st.R) / (2.0 * dist * sR + bE), dist


def attention_bwd_truth(qkv, dO_full, B):
    q = qkv.clone().requires_grad_(True)
    o, _, _ = attention(q, B)
    o.backward(dO_full)
    return q.grad


def attention_bwd_heads(q, k, v, g, delta, lse, scale=0.125):
    """attn_bwd on (..., T, 64) heads of any T: dQ, dK, dV from delta and lse (..., T), P / 8 and dS / 8 rounded to bf16 as MFMA operands.
    The kernel's factor is 2^-3, folded into the exponent offset and the dV store; `scale` enters the exponent alone, as the kernel's
    argument does (rovit_attention_bwd refuses any value but 1/8: dQ and dK would be 0.125 / scale times the truth)."""
    ps = torch.exp2((q @ k.transpose(-2, -1)) * (scale * LOG2E) - (lse + 3.0).unsqueeze(-1)).float().double()     # an fp32 number: it underflows
    dss = ps * (g @ v.transpose(-2, -1) - delta.unsqueeze(-1))
    psb, dsb = bf(ps), bf(dss)
    return dsb @ k, dsb.transpose(-2, -1) @ q, 8.0 * (psb.transpose(-2, -1) @ g)


def attention_bwd_emulated(qkv, o, lse, dO_full, B):
    """attn_bwd: statistics from the forward's saved o and lse, P / 8 and dS / 8 rounded to bf16 as MFMA operands."""
    q, k, v = heads_of(qkv, B)
    g = dO_full.view(B, ROWS, HEADS, HD).transpose(1, 2)                                # (B,3,197,64)
    delta = (dO_full * o).view(B, ROWS, HEADS, HD).sum(-1).transpose(1, 2)              # (B,3,197)
    dq, dk, dv = attention_bwd_heads(q, k, v, g, delta, lse)
    return torch.cat([rows_of(dq, B), rows_of(dk, B), rows_of(dv, B)], dim=1)


def attention_cls_bwd_heads(q0, k, v, g, delta, lse, scale=0.125):
    """attn_cls_bwd_kernel on (..., T, 64) keys and values of any T: q0, g (..., 64) the class token's query and output gradient, delta and
    lse (...).  Nothing is rounded before the outputs; the kernel honours its scale argument."""
    p = torch.exp2((k @ q0.unsqueeze(-1)).squeeze(-1) * (scale * LOG2E) - lse.unsqueeze(-1))          # (..., T)
    ds = p * ((v @ g.unsqueeze(-1)).squeeze(-1) - delta.unsqueeze(-1))
    dk = scale * ds.unsqueeze(-1) * q0.unsqueeze(-2)
    dv = p.unsqueeze(-1) * g.unsqueeze(-2)
    dq = torch.zeros_like(k)
    dq[..., 0, :] = scale * (ds.unsqueeze(-1) * k).sum(-2)
    return dq, dk, dv


def attention_cls_bwd_emulated(qkv, o_cls, lse_cls, dO_cls, B):
    """attn_cls_bwd_kernel: the class token's query alone, fp32 probabilities; dQ of every other query is zero."""
    q, k, v = heads_of(qkv, B)
    g = dO_cls.view(B, HEADS, HD)
    delta = (dO_cls * o_cls).view(B, HEADS, HD).sum(-1)                                  # (B,3)
    dq, dk, dv = attention_cls_bwd_heads(q[:, :, 0], k, v, g, delta, lse_cls.view(B, HEADS))
    return torch.cat([rows_of(dq, B), rows_of(dk, B), rows_of(dv, B)], dim=1)


def final_norm_bwd(run, sd):
    """The fp32 gradient entering the last block's class-token rows: the final norm's backward of d_features (nothing in it is rounded)."""
    g = run['dfeat'] * sd['norm.weight'].double()
    return ln_bwd(g, run['xhat_cls'], run['rstd_cls'])


def block_stages(run, sd, i):
    """The Stage records of block i: dx_in (last block only), dpre, dx_mid, dO, dqkv_q / _k / _v, dx_out."""
    B, depth = run['B'], run['depth']
    f, b, w = run['fwd'][i], run['bwd'][i], block_weights(sd, i)
    last = i == depth - 1
    out = []
    resid_R = resid_E = b['dx_in']
    if last:
        # plain fp32 arithmetic rounded once: REL plus half a bf16 ulp of the row's largest element
        resid_R = resid_E = final_norm_bwd(run, sd)
        out.append(Stage('dx_in', i, b['dx_in'], resid_R, resid_E, HALF_ULP * row_scale(resid_E)))
    # A1 (EPI_MUL): one bf16 ulp of the staged fc2 dgrad through the multiply by gelu'
    t_R, t_E = b['dx_in'] @ w['fc2'], bf(b['dx_in'] @ w['fc2_f'])
    out.append(Stage('dpre', i, b['dpre'], t_R * f['dact'], t_E * f['dact'], ULP * t_E.abs().amax(1) * f['dact'].abs().amax(1)))
    # A2 (EPI_LNBWD / the fused kernels' row pass): one bf16 ulp of the staged fc1 dgrad times rstd2, as test_gpu_block_bwd has it.  Row-wise
    # the output's own rounding needs a term the tensor-wise form did not: where the residual gradient dominates the row, half a bf16 ulp of
    # the output (2^-8 of the row's largest element) is more than REL of it, and the staged term, which scales with the branch, is small.
    v_R, v_E = b['dpre'] @ w['fc1_g'], bf(b['dpre'] @ w['fc1_f'])
    mid_R, mid_E = resid_R + ln_bwd(v_R, f['xhat2'], f['rstd2']), resid_E + ln_bwd(v_E, f['xhat2'], f['rstd2'])
    out.append(Stage('dx_mid', i, b['dx_mid'], mid_R, mid_E, ULP * v_E.abs().amax(1) * f['rstd2'] + HALF_ULP * row_scale(mid_E)))
    # A3 (EPI_BF16): a plain GEMM output
    o_R, o_E = b['dx_mid'] @ w['proj'], b['dx_mid'] @ w['proj_f']
    out.append(Stage('dO', i, b['dO'], o_R, o_E, HALF_ULP * row_scale(o_E)))
    # A4: each third of dqkv on its own row scale
    if last:
        dO_full = cls_to_full(b['dO'], B)
        q_E = attention_cls_bwd_emulated(f['qkv'], f['attn_o'], f['lse'], b['dO'], B)
    else:
        dO_full = b['dO']
        q_E = attention_bwd_emulated(f['qkv'], f['attn_o'], f['lse'], b['dO'], B)
    q_R = attention_bwd_truth(f['qkv'], dO_full, B)
    for k, n in enumerate(('dqkv_q', 'dqkv_k', 'dqkv_v')):
        sl = slice(D * k, D * (k + 1))
        out.append(Stage(n, i, b['dqkv'][:, sl], q_R[:, sl], q_E[:, sl], None, kind='R'))
    # A5: as A2, on dqkv and norm1 (in the last block the mid-block gradient is zero off the class-token rows)
    mid = cls_to_full(b['dx_mid'], B) if last else b['dx_mid']
    u_R, u_E = b['dqkv'] @ w['qkv_g'], bf(b['dqkv'] @ w['qkv_f'])
    x_R, x_E = mid + ln_bwd(u_R, f['xhat1'], f['rstd1']), mid + ln_bwd(u_E, f['xhat1'], f['rstd1'])
    out.append(Stage('dx_out', i, b['dx_out'], x_R, x_E, ULP * u_E.abs().amax(1) * f['rstd1'] + HALF_ULP * row_scale(x_E)))
    return out


# ---- the two saved fields only the backward reads ---------------------------------------------------------------------------------

def dact_ratio(run, sd, i, got=None):
    """got / bound per element of block i's gelu' against gelu'(fc1(norm2 affine(xhat2))) on the master weights.  Bound: half a bf16 ulp of
    the value plus max |gelu''| x the row's largest |pre_E - pre_R|, pre_E the bf16-staged pre-activation of the folded bf16 weights (the
    kernels' GELU input).  One term more than that: where the unrounded pre-activation lies within the fp32 accumulation error
    ((192 + 2) 2^-24 sum |terms|) of a rounding tie, the kernel may stage the other bf16 neighbour, and that element is allowed the
    neighbour's distance from pre_R instead."""
    f, w = run['fwd'][i], block_weights(sd, i)
    got = f['dact'] if got is None else got
    pre_R = (f['xhat2'] * w['fc1_gamma'] + w['fc1_beta']) @ w['fc1'].t() + w['fc1_b']
    pre_u = f['xhat2'] @ w['fc1_f'].t() + w['fc1_bf']
    pre_E = bf(pre_u)
    bits = pre_E.to(torch.bfloat16).view(torch.int16)
    other = (bits + torch.where(pre_u.abs() > pre_E.abs(), 1, -1).to(torch.int16)).view(torch.bfloat16).double()
    acc = (D + 2) * 2.0 ** -24 * (f['xhat2'].abs() @ w['fc1_f'].abs().t() + w['fc1_bf'].abs())
    near_tie = (pre_u - 0.5 * (pre_E + other)).abs() <= acc
    d_E = (pre_E - pre_R).abs()
    d_pre = torch.maximum(d_E.amax(1, keepdim=True).expand_as(d_E), torch.where(near_tie, (other - pre_R).abs(), d_E))
    ref = gelu_grad(pre_R)
    return (got - ref).abs() / (HALF_ULP * ref.abs() + GELU2_MAX * d_pre)


def lse_error(run, i, got=None):
    """|lse - log2-sum-exp of the engine's own qkv| per (image, head, query) (the last block: query 0)."""
    f = run['fwd'][i]
    got = f['lse'] if got is None else got
    ref = attention(f['qkv'], run['B'])[1]
    if got.shape[-1] == 1:
        ref = ref[:, :, :1]
    return (got - ref).abs()


# ---- parameter gradients ----------------------------------------------------------------------------------------------------------

def _splits(M, cap):
    return min(cap, (M + 63) // 64)


def _wgrad(dy, a, cap):
    """G = dy^T a, the column sums of dy, their sums of |terms| and the factor (n_terms + splits + 2) 2^-23."""
    M = dy.shape[0]
    return dy.t() @ a, dy.sum(0), dy.abs().t() @ a.abs(), dy.abs().sum(0), M, _splits(M, cap)


def _plain(out, name, dy, a, cap):
    G, cb, aG, acb, M, S = _wgrad(dy, a, cap)
    out[name + '.weight'] = (G, (M + S + 2) * U32 * aG)
    out[name + '.bias'] = (cb, (M + S + 2) * U32 * acb)


def _folded(out, name, norm, dy, a, W, gamma, beta, cap):
    """wgrad_reduce_batch_kernel's un-fold (the formulas of test_gpu_kernels.test_wgrad): with W_f = W gamma and b_f = b + W beta,
    dW = gamma G + beta (x) db, dgamma = sum_n W G, dbeta = sum_n W db; the column sums run over the N output rows on top of the M terms."""
    G, cb, aG, acb, M, S = _wgrad(dy, a, cap)
    N = W.shape[0]
    out[name + '.weight'] = (gamma * G + beta * cb[:, None], (M + S + 2) * U32 * (gamma.abs() * aG + beta.abs() * acb[:, None]))
    out[name + '.bias'] = (cb, (M + S + 2) * U32 * acb)
    out[norm + '.weight'] = ((W * G).sum(0), (M + N + S + 2) * U32 * (W.abs() * aG).sum(0))
    out[norm + '.bias'] = ((W * cb[:, None]).sum(0), (M + N + S + 2) * U32 * (W.abs() * acb[:, None]).sum(0))


def grad_refs(run, sd, x):
    """{parameter name: (fp64 reference from the engine's own buffers, per-element bound)}.  The products are exact in fp32 (bf16 x bf16), so
    only the fp32 accumulation errs: at most (n_terms + splits + 2) 2^-23 sum |terms| per element -- n_terms additions inside a split (M
    token rows; M plus the 768- or 576-term column sum for dgamma / dbeta), `splits` more in the reduce (at most 16 M-splits of 64-row
    steps in a block's merged launch, 4 in the last block's class-token launch, 32 for the patch embedding), 2 for the un-fold's multiply-add.
    'x.grad' is the image gradient when the run has one."""
    B, depth = run['B'], run['depth']
    out = {}
    for i in range(depth):
        f, b, w = run['fwd'][i], run['bwd'][i], block_weights(sd, i)
        cap = 4 if i == depth - 1 else 16
        pre = f'blocks.{i}.'
        part = {}
        _plain(part, 'mlp.fc2', b['dx_in'], f['act'], cap)
        _folded(part, 'mlp.fc1', 'norm2', b['dpre'], f['xhat2'], w['fc1'], w['fc1_gamma'], w['fc1_beta'], cap)
        _plain(part, 'attn.proj', b['dx_mid'], f['attn_o'], cap)
        _folded(part, 'attn.qkv', 'norm1', b['dqkv'], f['xhat1'], w['qkv'], w['qkv_gamma'], w['qkv_beta'], 16)
        out.update({pre + k: v for k, v in part.items()})
    # the final norm (cls_ln_affine_grad_kernel: fp32 x fp32 products, 16 batch slices)
    n = B + min(B, 16) + 2
    out['norm.weight'] = ((run['dfeat'] * run['xhat_cls']).sum(0), n * U32 * (run['dfeat'] * run['xhat_cls']).abs().sum(0))
    out['norm.bias'] = (run['dfeat'].sum(0), n * U32 * run['dfeat'].abs().sum(0))
    # from block 0's dx_out: pos_embed per token row (pos_grad_kernel: 4 batch slices), cls_token, the patch embedding
    g0 = run['bwd'][0]['dx_out'].view(B, ROWS, D)
    n = B + min(B, 4) + 2
    out['pos_embed'] = (g0.sum(0).view(1, ROWS, D), n * U32 * g0.abs().sum(0).view(1, ROWS, D))
    out['cls_token'] = (g0[:, 0].sum(0).view(1, 1, D), n * U32 * g0[:, 0].abs().sum(0).view(1, 1, D))
    dy, col = g0[:, 1:].reshape(-1, D), bf(patches(x))
    part = {}
    _plain(part, 'patch_embed.proj', dy, col, 32)
    out['patch_embed.proj.weight'] = tuple(t.view(D, 3, 16, 16) for t in part['patch_embed.proj.weight'])
    out['patch_embed.proj.bias'] = part['patch_embed.proj.bias']
    if run.get('xgrad') is not None:
        wpe = sd['patch_embed.proj.weight'].reshape(D, 768).to(torch.bfloat16).double()
        fold = lambda t: F.fold(t.view(B, 196, 768).transpose(1, 2), 224, 16, stride=16)    # noqa: E731
        out['x.grad'] = (fold(dy @ wpe), (D + 2) * U32 * fold(dy.abs() @ wpe.abs()))
    return out


def grad_ratio(got, ref, bound):
    """|got - ref| / bound per element; an element whose bound is zero (every term zero) must be exactly the reference."""
    err = (got.double() - ref).abs()
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))


def worst_of(ratio):
    """The largest ratio, its row and its column (NaN if any element is not finite).  Rows: the leading dimension, or for a tensor whose
    leading dimension is 1 (pos_embed, a vector) everything but the last one."""
    if ratio.dim() > 1 and ratio.shape[0] > 1:
        r = ratio.reshape(ratio.shape[0], -1)
    else:
        r = ratio.reshape(-1, ratio.shape[-1])
    if not torch.isfinite(r).all():
        return float('nan'), -1, -1
    k = int(r.argmax())
    return float(r.flatten()[k]), k // r.shape[1], k % r.shape[1]


# ---- the whole comparison ---------------------------------------------------------------------------------------------------------

def check_run(run, sd, x, label=''):
    """Every comparator on a run.  Returns (report, failures): report maps a field or parameter family to the worst ratio to its bound with
    the block and row (column) it occurs at, and the attention backward's E-to-R distances; failures lists what exceeds its bound."""
    report, fails = {}, []

    def note(key, val, where):
        old = report.get(key)
        if old is None or val != val or (old[0] == old[0] and val > old[0]):
            report[key] = (val, where)
        if not val <= 1.0:
            fails.append((key, val, where))

    for i in range(run['depth']):
        v, r, c = worst_of(dact_ratio(run, sd, i))
        note('dact', v, (i, r, c))
        e = lse_error(run, i)
        v, r, c = worst_of(e.reshape(-1, e.shape[-1]) / LSE_TOL)
        note('lse', v, (i, r, c))
        for st in block_stages(run, sd, i):
            rE, rR, dist = stage_ratios(st)
            if rE is not None:
                v, r, _ = worst_of(rE.unsqueeze(1))
                note(st.name + ' vs E', v, (i, r))
            v, r, _ = worst_of(rR.unsqueeze(1))
            note(st.name + ' vs R', v, (i, r))
            key = st.name + ' E-R distance'
            if key not in report or dist > report[key][0]:
                report[key] = (dist, (i,))
    for name, (ref, bound) in grad_refs(run, sd, x).items():
        got = run['xgrad'] if name == 'x.grad' else run['grads'][name]
        v, r, c = worst_of(grad_ratio(got, ref, bound))
        family = name.split('.', 2)[2] if name.startswith('blocks.') else name
        note('grad ' + family, v, (name, r, c))
    if label:
        print(f'{label}: worst ratio to the bound (block / parameter, row, column)')
        for k in sorted(report):
            print(f'    {k:28s} {report[k][0]:.3e}  {report[k][1]}')
    return report, fails


# ---- a CPU stand-in for the engine: E in the kernels' place -----------------------------------------------------------------------

def emulate_run(sd, x, w, depth, want_dx=False):
    """A run as the engine would leave it, computed on the CPU in fp64 with the kernels' roundings: the forward's saved fields, then the
    backward chained through bf16(E) of every stage, and parameter gradients as the fp32 rounding of the exact sums."""
    B = x.shape[0]
    M = B * ROWS
    sd64 = {k: v.double() for k, v in sd.items()}
    run = {'depth': depth, 'B': B, 'fwd': [], 'bwd': [None] * depth, 'dfeat': w.double(), 'grads': {}, 'xgrad': None}
    with torch.no_grad():
        t = ref_cpu.vit_embed(bf(x.double()), sd64).reshape(M, D)
        for i in range(depth):
            wt, f = block_weights(sd, i), {}
            last = i == depth - 1
            xh, f['rstd1'] = ln(t)
            f['xhat1'] = bf(xh)
            f['qkv'] = bf(f['xhat1'] @ wt['qkv_f'].t() + wt['qkv_bf'])
            o, lse, _ = attention(f['qkv'], B)
            o = bf(o)
            if last:
                o, lse, t = o.view(B, ROWS, D)[:, 0], lse[:, :, :1], t.view(B, ROWS, D)[:, 0]
            f['attn_o'], f['lse'] = o, lse.float().double()
            t = t + bf(o @ wt['proj_f'].t() + wt['proj_b'])
            xh, f['rstd2'] = ln(t)
            f['xhat2'] = bf(xh)
            pre = bf(f['xhat2'] @ wt['fc1_f'].t() + wt['fc1_bf'])
            f['act'], f['dact'] = bf(gelu(pre)), bf(gelu_grad(pre))
            t = t + bf(f['act'] @ wt['fc2_f'].t() + wt['fc2_b'])
            f['rstd1'], f['rstd2'] = f['rstd1'].float().double(), f['rstd2'].float().double()
            run['fwd'].append(f)
        xh, rs = ln(t)
        run['xhat_cls'], run['rstd_cls'] = xh.float().double(), rs.float().double()
    # the backward: every stage's output is bf16(E) of the stage, fed to the next
    dx = bf(final_norm_bwd(run, sd))
    for i in range(depth - 1, -1, -1):
        f, wt = run['fwd'][i], block_weights(sd, i)
        last = i == depth - 1
        b = {'dx_in': dx}
        resid = final_norm_bwd(run, sd) if last else dx
        b['dpre'] = bf(bf(dx @ wt['fc2_f']) * f['dact'])
        b['dx_mid'] = bf(resid + ln_bwd(bf(b['dpre'] @ wt['fc1_f']), f['xhat2'], f['rstd2']))
        b['dO'] = bf(b['dx_mid'] @ wt['proj_f'])
        with torch.no_grad():
            if last:
                b['dqkv'] = bf(attention_cls_bwd_emulated(f['qkv'], f['attn_o'], f['lse'], b['dO'], B))
            else:
                b['dqkv'] = bf(attention_bwd_emulated(f['qkv'], f['attn_o'], f['lse'], b['dO'], B))
        mid = cls_to_full(b['dx_mid'], B) if last else b['dx_mid']
        b['dx_out'] = bf(mid + ln_bwd(bf(b['dqkv'] @ wt['qkv_f']), f['xhat1'], f['rstd1']))
        run['bwd'][i] = b
        dx = b['dx_out']
    if want_dx:
        run['xgrad'] = 0          # placeholder: grad_refs() then includes 'x.grad'
    refs = grad_refs(run, sd, x)
    if want_dx:
        run['xgrad'] = refs.pop('x.grad')[0].float().double()
    run['grads'] = {k: v[0].float().double() for k, v in refs.items()}
    return run

"""Float64 reference of the contrastive token loss on the last-layer states (the rule: include/mmtg_hip.h at mmtg_cl_fwd) and the
bounds a correct fp32 evaluation of it stays inside.  Inputs come in their storage type and are widened exactly.

Bounds: e = 2^-24 is the unit roundoff of fp32 (one rounded operation has relative error <= e; a fused multiply-add counts as one);
first-order terms are written out, the factor SLACK = 1.01 covers the products of two of them (every relative error below is < 4e-5).
D = row length, n = kept positions of the sample, all quantities of the float64 reference unless marked ^ (the kernel's).

  norm      q^ = sum of D squares in fp32, any fixed order (all terms >= 0):  |q^ - q| <= D e q;  sqrt halves the relative error and
            adds e, the reciprocal adds e:                      |rinv^ - rinv| <= er rinv,   er = (D / 2 + 3) e
  dot       D products (exact for bf16 operands, one rounding each for fp32) added in fp32 in an arbitrary fixed order:
                                                               |dot^ - dot| <= (D + 1) e sum_k |h_ik| |h_jk|
  products  w^ = fl(rinv_i^ rinv_j^):  relative 2 er + e;   s^ = fl(dot^ w^): one more e:
            E_s = rinv_i rinv_j (D + 1) e sum_k |h_ik h_jk| + |s| (2 er + 2 e)
  hinge     x^ = fl(fl(rho - 1) + s^) (fused or not):  E_x = E_s + e (|x| + 1)    <- the DECIDING GAP: the kernel's a_ij can differ
            from the reference's only where |x| <= E_x.  l = max(0, x):  E_l = E_x where x > -E_x, else 0 (both are exactly 0).
  sums      cl_row, n terms in any order:    E_row = sum_j E_l + n e sum_j l
            cl_sample, L rows then one division by the exact integer n (n - 1) < 2^24:
                                             E_smp = (sum_i E_row + (L + 2) e sum_i cl_row) / (n (n - 1))
            cl, B samples then one division: E_cl = sum_b E_smp / den + (B + 1) e cl
  gradient (rows without a pair inside the gap; the caller leaves the others out, or asserts there are none)
            u_j^ = fl(h_j rinv_j^): relative eu = er + e.   G = sum_j a_ij u_j on the fp32 matrix cores, A_i active terms (adding an
            exact 0 rounds nothing):        E_G = (eu + (A_i + 1) e) sum_j a_ij |u_jd|
            g = G * fl(2 / (n (n - 1))):    E_g = scale E_G + 2 e |g|
            p = g . u_i, D fused terms:     E_p = sum_d E_g |u_id| + (eu + D e) sum_d |g_d u_id|
            projection, the cancellation explicit -- t_d = g_d - p u_id is small against g_d where the cosines are high, and its
            error is not:                   E_t = E_g + |u_id| (E_p + |p| (eu + 2 e)) + e |t_d|
            inc = fl(fl(coef rinv_i^) t):   E_inc = coef rinv_i E_t + |inc| (er + 3 e)
  store     out = round_to_storage(fl(old + inc^)):  E_out = E_inc + (e_out + e) (|old + inc| + E_inc),  e_out = 2^-24 (f32), 2^-8 (bf16)
"""
import torch

E32 = 2.0 ** -24
EOUT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8}      # unit roundoffs: 24 and 8 significand bits
SLACK = 1.01


def forward(hf, keep, P, L, margin, batch_den):
    """hf [B, P + L, D] (storage type), keep [B, P + L] integer.  Everything of the forward in float64, with its bounds."""
    B, Tt, D = hf.shape
    assert Tt == P + L
    h = hf.double()[:, P:]
    valid = keep[:, P:] != 0
    n = valid.sum(-1)
    r = (h * h).sum(-1).sqrt()
    ok = valid & (r > 0)
    rinv = torch.where(ok, 1.0 / r.clamp(min=1e-300), torch.zeros_like(r))
    u = h * rinv[..., None]
    s = u @ u.transpose(1, 2)
    rho = float(torch.tensor(margin, dtype=torch.float32))              # the margin as the kernel receives it
    x = rho - 1.0 + s
    eye = torch.eye(L, dtype=torch.bool)[None]
    pair = valid[:, :, None] & valid[:, None, :] & ~eye
    er = (D / 2 + 3) * E32
    absdot = h.abs() @ h.abs().transpose(1, 2)
    E_s = SLACK * (rinv[:, :, None] * rinv[:, None, :] * (D + 1) * E32 * absdot + s.abs() * (2 * er + 2 * E32))
    E_x = E_s + E32 * (x.abs() + 1.0)
    live = pair & ok[:, :, None] & ok[:, None, :]                       # (a zero row has s = 0 exactly: x = rho - 1 <= 0, never active)
    act = live & (x > 0)
    l = torch.where(act, x, torch.zeros_like(x))
    E_l = torch.where(live & (x > -E_x), E_x, torch.zeros_like(x))
    near = live & (x.abs() <= E_x)                                      # pairs inside the deciding gap
    cl_row = l.sum(-1)
    nf = n.double()
    E_row = E_l.sum(-1) + nf[:, None] * E32 * cl_row
    den = (nf * (nf - 1)).clamp(min=1.0)
    two = n >= 2
    cl_sample = torch.where(two, cl_row.sum(-1) / den, torch.zeros_like(den))
    E_smp = torch.where(two, (E_row.sum(-1) + (L + 2) * E32 * cl_row.sum(-1)) / den, torch.zeros_like(den)) * SLACK
    cl = cl_sample.sum() / batch_den
    E_cl = E_smp.sum() / batch_den + (B + 1) * E32 * cl
    full = lambda v: torch.cat([torch.zeros(B, P, dtype=v.dtype), v], 1).reshape(-1)
    return {"B": B, "P": P, "L": L, "D": D, "n": n, "valid": valid, "ok": ok, "rinv_l": rinv, "u": u, "x": x, "act": act, "pair": pair,
            "near": near, "gap": E_x, "margin_dist": torch.where(live, x.abs(), torch.full_like(x, float("inf"))),
            "rinv": full(rinv), "allow_rinv": full(er * rinv * SLACK), "cl_row": full(cl_row), "allow_row": full(E_row * SLACK),
            "cl_sample": cl_sample, "allow_sample": E_smp, "cl": cl, "allow_cl": E_cl * SLACK, "er": er}


def backward(fw, coef):
    """inc [B, L, D] = coef * d(sum_b cl_sample)/d(hf) on the lyric rows in float64, its bound E_inc, and the rows [B, L] that receive
    an increment at all (in I_b, nonzero norm, n_b >= 2)."""
    n, u, rinv, er, D = fw["n"], fw["u"], fw["rinv_l"], fw["er"], fw["D"]
    a = fw["act"].double()
    nf = n.double()
    two = (n >= 2)[:, None] & fw["ok"]
    scale = torch.where(n >= 2, 2.0 / (nf * (nf - 1)).clamp(min=1.0), torch.zeros_like(nf))[:, None, None]
    eu = er + E32
    G = a @ u
    A = a.sum(-1, keepdim=True)
    E_G = (eu + (A + 1) * E32) * (a @ u.abs())
    g = scale * G
    E_g = scale * E_G + 2 * E32 * g.abs()
    p = (g * u).sum(-1, keepdim=True)
    E_p = (E_g * u.abs()).sum(-1, keepdim=True) + (eu + D * E32) * (g * u).abs().sum(-1, keepdim=True)
    t = g - p * u
    E_t = E_g + u.abs() * (E_p + p.abs() * (eu + 2 * E32)) + E32 * t.abs()
    cr = coef * rinv[..., None]
    inc = cr * t
    E_inc = SLACK * (cr * E_t + inc.abs() * (er + 3 * E32))
    z = torch.zeros_like(inc)
    return torch.where(two[..., None], inc, z), torch.where(two[..., None], E_inc, z), two


def out_allow(old, inc, E_inc, out):
    """The bound on dhf after the add, for old (float64 of the stored pre-fill) and the storage type `out` of dhf."""
    return E_inc + (EOUT[out] + E32) * ((old + inc).abs() + E_inc) * SLACK


def gap_rows(fw):
    """Rows [B, L] with at least one pair inside the deciding gap (reference and kernel may disagree about a_ij there)."""
    return fw["near"].any(-1)


# ---------------------------------------------------------------- planted clusters: the inputs of tests/test_cl_ops_gpu.py
# (B, P, L, D): the smallest shapes at which a tile, sweep or mask edge can go wrong
SHAPES = [(1, 0, 1, 32),         # n = 1: every output 0, dhf untouched
          (2, 3, 2, 32),         # the smallest pair: sample 0 on one centre (active), sample 1 on two (inactive)
          (3, 2, 17, 64),        # one past a 16-row tile
          (4, 15, 33, 768),      # the model's D; keep: all kept, every third column PAD, n_b = 1, n_b = 0
          (2, 1, 65, 1024),      # one past a 64-column sweep, the largest D
          (1, 15, 221, 768)]     # the fixture's own L = 13 x 16 + 13
MARGINS = (0.5, 0.25)


def planted(shape, dtype, seed=0):
    """Row i of a sample is centre[i % 3] + 0.3 gaussian / sqrt(D), times a row scale in [0.5, 4.5]; the three centres are
    orthonormal; the values are rounded to `dtype`.  Pairs on one centre have a cosine near 0.92, pairs on two near 0: for the
    margins 0.5 and 0.25 every rho - 1 + s_ij is far from 0 (the caller asserts it against the deciding gap).  From L = 17 up row
    (0, 5) is zero.  Returns hf [B, P + L, D] and keep [B, P + L] int32 (topic columns kept, as the forward's mask has them)."""
    B, P, L, D = shape
    gen = torch.Generator().manual_seed(1000 * seed + 7 * L + D)
    centres = torch.linalg.qr(torch.randn(D, 3, generator=gen, dtype=torch.float64))[0].T
    Tt = P + L
    idx = torch.arange(Tt) % 3
    hf = centres[idx][None].repeat(B, 1, 1)
    if L == 2:
        hf[0] = centres[0]
    hf = hf + 0.3 * torch.randn(B, Tt, D, generator=gen, dtype=torch.float64) / D ** 0.5
    hf = hf * (0.5 + 4.0 * torch.rand(B, Tt, 1, generator=gen, dtype=torch.float64))
    keep = torch.ones(B, Tt, dtype=torch.int32)
    if B == 4:
        keep[1, P::3] = 0
        keep[2, P:] = 0
        keep[2, P + 4] = 1
        keep[3, P:] = 0
    elif B == 3:
        keep[1, Tt - 3:] = 0
    zero_row = (0, 5) if L >= 17 else None
    if zero_row is not None:
        hf[0, P + 5] = 0.0
    return hf.to(dtype), keep, zero_row

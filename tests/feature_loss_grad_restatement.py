"""A float64 statement of the training step's loss gradients (include/oryon_hip.h, oryon_feature_loss_grad / oryon_mask_dice_grad;
DESIGN.md "The training step"), in numpy, written from the definition and not from autograd.  Notation: feature_loss_restatement.py.

  cosine     for |u| >= eps: d<u^,v^>/du = (v^ - <u^,v^> u^) / |u|;  for |u| < eps the clamped norm is a constant: v^ / eps
  margins    strict: a row contributes through d_pos only if d_pos - m_pos > 0, through d_neg_s only if m_neg - d_neg_s > 0
  weights    alpha = g_pos / (V N), beta_s = -g_neg_s / (V N); V = number of pairs with valid == 1
  slots      per pair and side (u_n the side's positive, v_n the other side's, w_n the side's negative, its index a constant):
                 slot n     at the positive's pixel: alpha d d_pos/du_n + beta_s d d(u_n,w_n)/du_n
                 slot N + n at the negative's pixel: beta_s d d(u_n,w_n)/dw_n
             G_s[b,:,y,x] = the sum of the slots at the pixel; every other element 0; an invalid pair: all 0
  dice       dL/dx_i = g (0.25 / B) 2 p_i q_i [(-t_i/D_f + 2 p_i (S_pt+1)/D_f^2) - (-u_i/D_b + 2 q_i (S_qu+1)/D_b^2)]

Besides G every function returns S, per element the sum of the magnitudes of the terms that were added into it (three terms per
correspondence: the two of slot n and the one of slot N + n): the scale against which an fp32 evaluation of the same sum errs."""
import numpy as np

import feature_loss_restatement as fr

EPS = fr.EPS


def dcos(u, v):
    """rows u, v [N,C] -> (d<u^,v^>/du [N,C], <u^,v^> [N])."""
    lu = np.sqrt((u * u).sum(1, keepdims=True))
    nu = np.maximum(lu, EPS)
    uh, vh = u / nu, fr.unit(v)
    c = (uh * vh).sum(1, keepdims=True)
    return (vh - np.where(lu >= EPS, c, 0.0) * uh) / nu, c[:, 0]


def map_grads(feat_a, feat_q, pix, valid, neg_idx, g, pos_margin=0.2, neg_margin=0.9, d_pos=None, d_neg=None, slots=None):
    """feat_* [B,C,FH,FW], pix [B,N,4] feature pixels, neg_idx [B,2,N] linear pixels (outside the map: no pixel), g = (g_pos, g_neg_a,
    g_neg_q) -> (G [2,B,C,FH,FW], S [2,B,C,FH,FW], active [B,3,N] bool = rows inside the margins (pos, neg_a, neg_q)).
    d_pos [B,N] / d_neg [B,2,N]: the distances the margins are tested on (default: the float64 ones).
    slots: a dict that receives, per (side, b) of a valid pair, (keys [2 N] linear pixels or -1, values [2 N, C]): the 2 N slots."""
    feat = (np.asarray(feat_a, dtype=np.float64), np.asarray(feat_q, dtype=np.float64))
    B, C, FH, FW = feat[0].shape
    HW, N = FH * FW, pix.shape[1]
    G, S = np.zeros((2, B, C, HW)), np.zeros((2, B, C, HW))
    active = np.zeros((B, 3, N), dtype=bool)
    V = int(sum(1 for v in valid if v == 1))
    for b in range(B):
        if valid[b] != 1:
            continue
        rows = [feat[s][b].reshape(C, HW).T for s in (0, 1)]
        key = [pix[b, :, 0] * FW + pix[b, :, 1], pix[b, :, 2] * FW + pix[b, :, 3]]
        pos = [rows[s][key[s]] for s in (0, 1)]
        for s in (0, 1):
            u, v = pos[s], pos[1 - s]
            wi = np.asarray(neg_idx[b, s], dtype=np.int64)
            has_w = (wi >= 0) & (wi < HW)
            w = np.where(has_w[:, None], rows[s][np.where(has_w, wi, 0)], 0.0)
            du_pos, c_uv = dcos(u, v)
            du_neg, c_uw = dcos(u, w)
            dw_neg, _ = dcos(w, u)
            dp = 0.5 * (1.0 - c_uv) if d_pos is None else np.asarray(d_pos[b], dtype=np.float32)
            dn = 0.5 * (1.0 - c_uw) if d_neg is None else np.asarray(d_neg[b, s], dtype=np.float32)
            if d_pos is None:
                a_pos = dp - pos_margin > 0
            else:
                a_pos = dp - np.float32(pos_margin) > 0
            a_neg = (neg_margin - dn > 0) if d_neg is None else (np.float32(neg_margin) - dn > 0)
            active[b, 0], active[b, 1 + s] = a_pos, a_neg
            alpha = np.where(a_pos, g[0] / (V * N), 0.0)[:, None]
            beta = np.where(a_neg, -g[1 + s] / (V * N), 0.0)[:, None]
            t_pos, t_neg, t_w = alpha * (-0.5 * du_pos), beta * (-0.5 * du_neg), beta * (-0.5 * dw_neg)
            np.add.at(G[s, b].T, key[s], t_pos + t_neg)
            np.add.at(S[s, b].T, key[s], np.abs(t_pos) + np.abs(t_neg))
            np.add.at(G[s, b].T, wi[has_w], t_w[has_w])
            np.add.at(S[s, b].T, wi[has_w], np.abs(t_w[has_w]))
            if slots is not None:
                slots[s, b] = (np.concatenate([key[s], np.where(has_w, wi, -1)]), np.concatenate([t_pos + t_neg, np.where(has_w[:, None], t_w, 0.0)]))
    shape = (2, B, C, FH, FW)
    return G.reshape(shape), S.reshape(shape), active


def touched(pix, valid, neg_idx, feat_hw):
    """-> [2,B,FH,FW] bool: the pixels some slot of a valid pair sits at."""
    FH, FW = feat_hw
    B = pix.shape[0]
    out = np.zeros((2, B, FH * FW), dtype=bool)
    for b in range(B):
        if valid[b] != 1:
            continue
        for s in (0, 1):
            out[s, b, pix[b, :, 2 * s] * FW + pix[b, :, 2 * s + 1]] = True
            wi = np.asarray(neg_idx[b, s], dtype=np.int64)
            out[s, b, wi[(wi >= 0) & (wi < FH * FW)]] = True
    return out.reshape(2, B, FH, FW)


def dice_grad(logits, gt, g_mask):
    """logits [B,H,W], gt [B,H,W] at the same size, g_mask the gradient of this image set's dice loss -> (dL/dlogits [B,H,W], T [B,H,W]).
    T = |g| (0.25 / B) 2 (t/D_f + 2 p (S_pt+1)/D_f^2 + u/D_b + 2 q (S_qu+1)/D_b^2): the magnitudes of the four terms WITHOUT the factor
    p q.  An fp32 softmax backward forms p q (a - b) as p (a - (p a + q b)), so where the sigmoid saturates it errs on the scale of T,
    not of the gradient: the reference's recorded fp32 logit gradients can only be held against T."""
    x = np.asarray(logits, dtype=np.float64)
    B = len(x)
    t = (np.asarray(gt) != 0).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-2.0 * x))
    q, u = 1.0 - p, 1.0 - t
    ax = (1, 2)
    Df = ((p * p).sum(ax) + t.sum(ax) + 1.0)[:, None, None]
    Db = ((q * q).sum(ax) + u.sum(ax) + 1.0)[:, None, None]
    Nf = ((p * t).sum(ax) + 1.0)[:, None, None]
    Nb = ((q * u).sum(ax) + 1.0)[:, None, None]
    grad = g_mask * (0.25 / B) * 2.0 * p * q * ((-t / Df + 2.0 * p * Nf / Df ** 2) - (-u / Db + 2.0 * q * Nb / Db ** 2))
    return grad, abs(g_mask) * (0.25 / B) * 2.0 * (t / Df + 2.0 * p * Nf / Df ** 2 + u / Db + 2.0 * q * Nb / Db ** 2)

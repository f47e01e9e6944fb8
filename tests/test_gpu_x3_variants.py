"""The fp16x3 kernels at the shapes that select the instantiations and loop phases the workload-shaped tests never reach (DESIGN.md,
"Kernel variants and the shapes that reach them"):

  * linear_f16x3_stream_kernel: the hand-off between the tiles of a persistent workgroup's stream - second tiles, middle tiles, a
    half-wide column tile that is not first, nk = 2 / 3 / 5 (odd nk: the next tile starts on the other LDS stage), every
    <ACT, WEX, ACC> instantiation.  Which workgroup walks which tiles is PROVED per case with tests/x3_slot_map.py for the device's
    own CU count, and the bitwise comparison against one-tile-per-workgroup calls of the same rows turns a stale stage of any size
    into a failure.
  * mha_x3_kernel: the three tile bodies at every remainder class of L, query blocks with 1-4 live waves.
  * dec_conv3x3_kernel<1, false, IN_GN, true>: the persistent register-weight convolution against the one-item-per-workgroup variant.
  * swin_window_attention_x3_kernel on fp32 tensors, directly, at odd map sizes.
References are float64 torch; the bars are the ones tests/test_backbone_pins.py and tests/test_gpu_decoder.py hold the same kernels to."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_slot_map as sm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. stream GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
def _has_depth(d):
    return lambda st, geo: any(len(s) >= d and sm.is_ragged_m(s[-1], geo) for s in st)


def _half_wide_not_first(st, geo):
    return any(len(s) >= 2 and any(sm.is_half_wide(t, geo) for t in s[1:]) for s in st)


def _half_wide_middle(st, geo):
    return _has_depth(3)(st, geo) and any(len(s) >= 3 and any(sm.is_half_wide(t, geo) for t in s[1:-1]) for s in st)


# (M on a 256-CU device, N) -> the class the case claims: what some workgroup's stream must look like
GEMM_CLASSES = {
    (8449, 256): ("two tiles, the ragged-M tile second", _has_depth(2)),
    (8449, 128): ("two tiles of a single half-wide column", _has_depth(2)),
    (4353, 384): ("two tiles, a half-wide tile second", lambda st, geo: _has_depth(2)(st, geo) and _half_wide_not_first(st, geo)),
    (16540, 2048): ("three tiles, the ragged-M tile last", _has_depth(3)),
    (16540, 1920): ("three tiles, a half-wide middle tile", _half_wide_middle),
}
GEMM_CASES = ([(M, K, N) for (M, N) in ((8449, 256), (8449, 128), (4353, 384)) for K in (64, 96, 160)]
              + [(M, K, N) for (M, N) in ((16540, 2048), (16540, 1920)) for K in (64, 96)])


def _rows_for_device(M, N):
    """The issue's M where this device's plan has the class; otherwise the smallest M (searched over tiles_m) that has it."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    name, want = GEMM_CLASSES[(M, N)]
    geo = sm.geometry(M, N)
    if not want(sm.plan_for_cus(M, N, cus), geo):
        M = sm.find_m(N, cus, want, m_max=40000)
        assert M is not None, f"no M <= 40000 gives '{name}' at N = {N} on {cus} CUs"
        geo = sm.geometry(M, N)
    streams = sm.plan_for_cus(M, N, cus)
    assert want(streams, geo), (name, M, N, cus)
    return M, streams, geo


def _act(y, act):
    if act == "erf":
        return F.gelu(y)
    if act == "quick":
        return y * torch.sigmoid(1.702 * y)
    return y


@pytest.mark.parametrize("M256,K,N", GEMM_CASES)
def test_stream_gemm_tile_handoff_every_instantiation(M256, K, N):
    """Per case: the plan proves the class; then for act in {none, quick, erf} x {general, fp16-exact weights} and the accumulate entry
    x {general, exact}:  (a) fp64 bar of test_fp16x3_linear_and_clip_tower_match_fp32 (< 5e-6 and <= 2 e_32 + 1e-7 of max |ref|),
    (b) every 256-row block owned by a multi-tile workgroup, and the ragged last block, equals bit for bit the stand-alone call on those
    rows (one tile per workgroup: prologue, no hand-off), (c) W_lo = NULL equals the three-product kernel bit for bit, (d) the
    accumulate entry equals c0 + linear bit for bit, (e) the range flag stays clear."""
    from oryon_amd import ops
    torch.backends.cuda.matmul.allow_tf32 = False
    M, streams, geo = _rows_for_device(M256, N)
    nk = K // 32
    assert nk in (2, 3, 5) and max(len(s) for s in streams) >= (3 if N >= 1920 else 2)
    multi_rows = sorted({tm for s in streams if len(s) > 1 for tm, _ in s} | {geo["tiles_m"] - 1})
    blocks = [(tm * 256, min(M, tm * 256 + 256)) for tm in multi_rows]
    assert M % 256 != 0 and blocks[-1][1] == M
    # a stand-alone call on <= 256 rows is one tile per workgroup on this device
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert all(len(s) <= 1 for r0, r1 in (blocks[0], blocks[-1]) for s in sm.plan_for_cus(r1 - r0, N, cus))
    g = torch.Generator(device=DEV).manual_seed(1000 * nk + N)
    with torch.no_grad():
        x = torch.randn(M, K, generator=g, device=DEV) * 3.0
        w_gen = torch.randn(N, K, generator=g, device=DEV) * K ** -0.5
        b = torch.randn(N, generator=g, device=DEV)
        c0 = torch.randn(M, N, generator=g, device=DEV) * 5.0
        w_ex = w_gen.half().float()
        rows = torch.cat([torch.arange(r0, r1, device=DEV) for r0, r1 in blocks])

        def blockwise(w, **kw):
            return torch.cat([ops.linear_f16x3(x[r0:r1], w, b, **kw) for r0, r1 in blocks])

        ops.x3_range_flag(DEV, reset=True)
        for exact, w in ((False, w_gen), (True, w_ex)):
            hi, lo = ops._split_weight_f16x3(w)
            assert (lo is None) == exact
            lin64 = F.linear(x.double(), w.double(), b.double())
            lin32 = F.linear(x, w, b)
            w3 = None
            if exact:
                ops.X3_EXACT_WEIGHTS = False
                try:
                    w3 = w.clone()
                    assert ops._split_weight_f16x3(w3)[1] is not None
                finally:
                    ops.X3_EXACT_WEIGHTS = True
            plain = None
            for act in (None, "quick", "erf"):
                kw = dict(quick_gelu=act == "quick", gelu=act == "erf")
                got = ops.linear_f16x3(x, w, b, **kw)
                ref, f32 = _act(lin64, act), _act(lin32, act)
                scale = float(ref.abs().max())
                e_x3, e_32 = float((got.double() - ref).abs().max()) / scale, float((f32.double() - ref).abs().max()) / scale
                del ref, f32
                print(f"gemm M={M} K={K} N={N} exact={exact} act={act}: e_x3={e_x3:.3e} e_32={e_32:.3e}")
                assert e_x3 < 5e-6 and e_x3 <= 2.0 * e_32 + 1e-7, (M, K, N, exact, act, e_x3, e_32)
                small = blockwise(w, **kw)
                bad = (got[rows] != small).any(dim=1)
                assert not bool(bad.any()), (M, K, N, exact, act, "rows that depend on their tile's place in the stream:", rows[bad][:8].tolist(),
                                             float((got[rows] - small).abs().max()))
                if exact:                                   # (c) the three-product kernel on the same (fp16-valued) weights
                    assert torch.equal(got, ops.linear_f16x3(x, w3, b, **kw)), (M, K, N, act)
                if act is None:
                    plain, plain_small = got, small
                assert ops.x3_range_flag(DEV) is False, (M, K, N, exact, act)
            # (d) accumulate: ACT = 0, ACC, WEX = exact
            assert ops.linear_f16x3_acc_supported(w, c0)
            buf = c0.clone()
            assert ops.linear_f16x3_acc(x, w, b, buf) is buf
            assert torch.equal(buf, c0 + plain), (M, K, N, exact, float((buf - (c0 + plain)).abs().max()))
            assert torch.equal(buf[rows], c0[rows] + plain_small), (M, K, N, exact)
            if exact:
                buf3 = c0.clone()
                ops.linear_f16x3_acc(x, w3, b, buf3)
                assert torch.equal(buf3, buf), (M, K, N)
            assert ops.x3_range_flag(DEV) is False, (M, K, N, exact, "acc")
            del lin64, lin32


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. multi-head attention
# ---------------------------------------------------------------------------------------------------------------------------------
def _mha_route(L):
    """mha_x3_kernel's dispatch restated: (body of the last key tile, its valid keys, whether it is the only tile, live waves of the last
    query block, queries in that block's last live wave)."""
    j0 = (L - 1) // 64 * 64
    if j0 + 64 <= L:
        body = "<2,false>"
    elif j0 + 32 < L:
        body = "<2,true>"
    else:
        body = "<1,true>"
    q0 = (L - 1) // 128 * 128
    live = sum(1 for wave in range(4) if q0 + wave * 32 < L)
    return body, L - j0, j0 == 0, live, L - (q0 + (live - 1) * 32)


# L -> what it reaches: last-tile body, valid keys in it, only tile?, live waves in the last query block, queries in the last live wave
MHA_ROUTES = {
    1: ("<1,true>", 1, True, 1, 1),            # one valid key of 32: every other score masked while m_run is still -inf
    31: ("<1,true>", 31, True, 1, 31),
    32: ("<1,true>", 32, True, 1, 32),         # exactly 32 keys: the boundary of `j0 + 32 < L`, nothing masked in the half tile
    33: ("<2,true>", 33, True, 2, 1),          # the ragged full-width body as the FIRST and only tile
    63: ("<2,true>", 63, True, 2, 31),
    96: ("<1,true>", 32, False, 3, 32),        # L % 64 == 32 behind a full tile; three live waves
    100: ("<2,true>", 36, False, 4, 4),        # the ragged full-width body as last tile
    127: ("<2,true>", 63, False, 4, 31),
    161: ("<2,true>", 33, False, 2, 1),        # two query blocks; the second has two live waves, one query in the last
    225: ("<2,true>", 33, False, 4, 1),
}


def test_mha_route_table_covers_every_body_and_remainder():
    assert all(_mha_route(L) == r for L, r in MHA_ROUTES.items())
    R = MHA_ROUTES
    assert all(R[L][0] == "<2,true>" and not R[L][2] and 33 <= L % 64 <= 63 for L in (100, 161, 225))
    assert all(R[L][0] == "<2,true>" and R[L][2] and 33 <= L % 64 <= 63 for L in (33, 63))
    assert sorted(R[L][1] for L in (1, 31, 32)) == [1, 31, 32] and all(R[L][0] == "<1,true>" for L in (1, 31, 32, 96)) and 96 % 64 == 32
    assert {r[3] for r in R.values()} == {1, 2, 3, 4} and any(r[4] < 32 for r in R.values())
    # the shapes of test_mha_f16x3_matches_fp64_attention, for comparison: none of them reaches <2,true>
    assert _mha_route(577) == ("<1,true>", 1, False, 3, 1) and _mha_route(64)[0] == "<2,false>" and _mha_route(130) == ("<1,true>", 2, False, 1, 2)


def _mha_ref(qkv, H, dtype):
    N, L, _ = qkv.shape
    q, k, v = qkv.view(N, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    if dtype == torch.float64:
        o = torch.softmax(q.double() @ k.double().transpose(-2, -1) / 8.0, dim=-1) @ v.double()
    else:
        o = F.scaled_dot_product_attention(q, k, v)
    return o.transpose(1, 2).reshape(N, L, 64 * H)


@pytest.mark.parametrize("L", sorted(MHA_ROUTES))
def test_mha_every_tile_body_and_remainder(L):
    """(N, H) = (1,1), (3,1), (2,4), (3,3): 1, 3, 8 and 9 units - the `unit >= n_units` exit of the padded grid and the XCD map.  fp64 bar
    of test_mha_f16x3_matches_fp64_attention, element by element as well, finite, and every (image, head) of the batched call equal bit
    for bit to the single-unit call on that head's q | k | v."""
    from oryon_amd import ops
    assert _mha_route(L) == MHA_ROUTES[L]
    g = torch.Generator(device=DEV).manual_seed(100 + L)
    with torch.no_grad():
        for N, H in ((1, 1), (3, 1), (2, 4), (3, 3)):
            D = 64 * H
            qkv = torch.randn(N, L, 3 * D, generator=g, device=DEV) * 1.5
            got = ops.mha_f16x3(qkv, H)
            assert got.shape == (N, L, D) and bool(torch.isfinite(got).all())
            ref, f32 = _mha_ref(qkv, H, torch.float64), _mha_ref(qkv, H, torch.float32)
            scale = float(ref.abs().max())
            e_x3, e_32 = float((got.double() - ref).abs().max()) / scale, float((f32.double() - ref).abs().max()) / scale
            print(f"mha L={L} N={N} H={H}: e_x3={e_x3:.3e} e_32={e_32:.3e}")
            assert e_x3 < 5e-6 and e_x3 <= 3.0 * e_32 + 2e-7, (N, L, H, e_x3, e_32)
            torch.testing.assert_close(got, ref.float(), rtol=1e-4, atol=1e-5 * scale)
            if (N, H) == (1, 1):
                continue
            for n in range(N):
                for h in range(H):
                    one = torch.cat([qkv[n:n + 1, :, t * D + h * 64:t * D + (h + 1) * 64] for t in range(3)], dim=-1).contiguous()
                    assert torch.equal(got[n:n + 1, :, h * 64:(h + 1) * 64], ops.mha_f16x3(one, 1)), (N, L, H, n, h)


@pytest.mark.parametrize("L", [33, 100, 225])
def test_mha_reads_nothing_past_the_last_row(L):
    """The ragged tile clamps rows past L to row L-1 instead of zeroing them: correct only if their p is exactly 0 AND nothing beyond row
    L-1 is ever loaded.  The sequence sits in front of 64 rows of NaN: an unclamped K or V read would put NaN into the products even
    under p = 0."""
    from oryon_amd import ops
    H = 2
    g = torch.Generator(device=DEV).manual_seed(7 + L)
    with torch.no_grad():
        big = torch.full((1, L + 64, 3 * 64 * H), float("nan"), device=DEV)
        big[:, :L] = torch.randn(1, L, 3 * 64 * H, generator=g, device=DEV) * 1.5
        view = big[:, :L]
        assert view.is_contiguous() and view.data_ptr() == big.data_ptr()
        got = ops.mha_f16x3(view, H)
        alone = ops.mha_f16x3(view.clone(), H)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, alone)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. decoder: the persistent register-weight convolution against the one-item-per-workgroup variant
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(3, 32, 24), (5, 48, 40)])
def test_decoder_batched_forward_equals_single_image_forwards_bitwise(n, h, w):
    """launch_conv (csrc/decoder.hip) sends a cin == cout == 32 convolution with n * tiles > 512 items to the persistent instantiation
    (weights in registers, items strided over 512 workgroups, streams crossing image boundaries, red[] re-used, unpredicated stores); the
    n = 1 forward of the same image has tiles <= 480 and takes the one-item-per-workgroup instantiation.  Both issue the same MFMA
    sequence on the same operands and share the epilogue and the GroupNorm partials (fixed order, per image): image i of the batched
    forward must equal the n = 1 forward of image i bit for bit - outputs and decoder3's three workspace intermediates."""
    from oryon_amd.backbone.decoder_hip import HipDecoder
    from test_gpu_decoder import _decoder, _nhwc, persistent_conv_items
    d2, d3 = persistent_conv_items(n, h, w)
    one2, one3 = persistent_conv_items(1, h, w)
    assert d3 > 512 and one2 <= 512 and one3 <= 512                # batched decoder3 persistent, every n = 1 convolution not
    assert (d2 > 512) == ((n, h, w) == (5, 48, 40))
    torch.manual_seed(21)
    dec = _decoder(13)
    x = torch.randn(n, 128, h, w, device=DEV)
    g2 = torch.randn(n, 256, 2 * h, 2 * w, device=DEV) * 2.0
    g3 = torch.randn(n, 128, 4 * h, 4 * w, device=DEV) * 0.5 + 0.3
    hip = HipDecoder(dec, x.device)
    H, W = 8 * h, 8 * w

    def run(xs, a2, a3):
        m = xs.shape[0]
        off = hip.layout(m, h, w)
        inter = []
        for stop in (7, 8, 9):                                     # decoder3: cat buffer, raw conv1, raw conv2
            hip.forward(xs, a2, a3, stop_after=stop)
            torch.cuda.synchronize()
            inter.append(_nhwc(hip.workspace(m, h, w), off[stop - 7], m, H, W, 32).clone())
        lg, fm = hip.forward(xs, a2, a3)
        return inter + [lg, fm]
    with torch.no_grad():
        batched = run(x, g2, g3)
        assert all(bool(torch.isfinite(t).all()) for t in batched)
        for i in range(n):
            single = run(x[i:i + 1], g2[i:i + 1], g3[i:i + 1])
            for name, a, s in zip(("cat3", "conv3a", "conv3b", "logits", "featmap"), batched, single):
                assert torch.equal(a[i:i + 1], s), (n, h, w, i, name, float((a[i:i + 1] - s).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the f32 Swin window attention, directly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,heads,H,W", [(128, 4, 20, 17), (256, 8, 14, 14), (64, 2, 7, 9)])
@pytest.mark.parametrize("shift", [0, 3])
def test_swin_window_attention_f32_kernel_vs_fp64_module(dim, heads, H, W, shift):
    """swin_window_attention_x3_kernel (fp32 I/O) inside swin._WindowAttention at the bf16 kernel's test shapes (maps that need window
    padding, one exact window row, shifts) against the same module evaluated in float64 on the plain path: < 5e-6 and <= 3 e_32 + 2e-7 of
    max |ref| (e_32 = the plain fp32 module), and element by element."""
    from oryon_amd import ops
    from oryon_amd.backbone import swin as swin_mod
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(31 + dim + shift)
    att = swin_mod._WindowAttention(dim, heads, 7, shift).to(DEV).eval()
    calls = []
    real = ops.swin_window_attention_f32
    with torch.no_grad():
        att.relative_position_bias_table.normal_(std=0.5)
        att.qkv.bias.normal_(std=0.3)
        x = torch.randn(2, H, W, dim, device=DEV)
        att64 = swin_mod._WindowAttention(dim, heads, 7, shift).to(DEV).double().eval()
        att64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in att.state_dict().items()})
        assert not swin_mod.FUSED_F32_ATTENTION
        ref = att64(x.double())
        f32 = att(x)
        ops.swin_window_attention_f32 = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        swin_mod.FUSED_F32_ATTENTION = True
        try:
            got = att(x)
        finally:
            swin_mod.FUSED_F32_ATTENTION = False
            ops.swin_window_attention_f32 = real
    assert calls == [1] and got.shape == ref.shape and got.dtype == torch.float32          # the kernel ran, once
    scale = float(ref.abs().max())
    e_x3, e_32 = float((got.double() - ref).abs().max()) / scale, float((f32.double() - ref).abs().max()) / scale
    print(f"swin f32 dim={dim} heads={heads} {H}x{W} shift={shift}: e_x3={e_x3:.3e} e_32={e_32:.3e}")
    assert e_x3 < 5e-6 and e_x3 <= 3.0 * e_32 + 2e-7, (dim, heads, H, W, shift, e_x3, e_32)
    torch.testing.assert_close(got, ref.float(), rtol=1e-4, atol=1e-5 * scale)

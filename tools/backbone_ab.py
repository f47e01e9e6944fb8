"""A/B of the backbone's fp16x3 kernels (window attentions, linears, CLIP attention, conv24, decoder) between two builds of the library.

  ORYON_DEVLIB=/path/to/liboryon_hip.so python tools/backbone_ab.py run out.npz    # one library, one process
  python tools/backbone_ab.py compare a.npz b.npz                                   # every array bit for bit
  ORYON_DEVLIB=/path/to/liboryon_hip.so python tools/backbone_ab.py time           # the two window kernels at their workload shapes

`run` feeds seeded CPU-generated inputs at small shapes to each kernel and writes the outputs.  `time` prints the median of 20
HIP-event-timed groups of ten calls of fusion_window_attention_x3_kernel (128 images, 24 x 24, C 128, 4 heads, shift 6) and of
swin_window_attention_x3_kernel (32 images, 96 x 96, dim 128, 4 heads, shift 3); alternate the two libraries, one process each."""
import sys

import numpy as np


def _inputs():
    import torch
    g = torch.Generator().manual_seed(29)
    rnd = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s
    return torch, rnd


def run(out_path):
    import _devlib  # noqa: F401
    torch, rnd = _inputs()
    from oracle import oryon_oracle as orc
    from oryon_amd import ops
    from oryon_amd.backbone.decoder_hip import HipDecoder
    from oryon_amd.backbone.fusion import StandardDecoder
    dev = torch.device("cuda", 0)
    out = {}

    def put(name, t):
        out[name] = t.cpu().numpy()
        assert np.isfinite(out[name]).all() and np.abs(out[name]).sum() > 0, name

    for B, H, W, C, heads, shifts in ((2, 24, 24, 64, 2, (0, 6)), (1, 12, 24, 128, 4, (5,))):
        qk, v = rnd(B, H, W, 2 * C, s=2.0).to(dev), rnd(B, H, W, C).to(dev)
        for shift in shifts:
            put(f"fusion_window/{B}x{H}x{W}_c{C}_s{shift}", ops.fusion_window_attention(qk, v, heads, 12, shift))
    for dim, heads, H, W in ((64, 2, 7, 9), (128, 4, 20, 17)):
        qkv, pad, bias = rnd(2, H, W, 3 * dim, s=1.5).to(dev), rnd(3 * dim, s=0.5).to(dev), rnd(heads, 49, 49).to(dev)
        for shift in (0, 3):
            put(f"swin_window/{H}x{W}_d{dim}_s{shift}", ops.swin_window_attention_f32(qkv, pad, bias, heads, shift))
    x64, x32 = rnd(300, 64).to(dev), rnd(300, 32).to(dev)
    w64, w32, b = rnd(256, 64, s=0.2).to(dev), rnd(256, 32, s=0.2).to(dev), rnd(256, s=0.1).to(dev)
    put("linear/k64_n256", ops.linear_f16x3(x64, w64, b))
    put("linear/k32_small_tile", ops.linear_f16x3(x32, w32, b))
    put("linear/k64_quick_gelu", ops.linear_f16x3(x64, w64, b, quick_gelu=True))
    put("linear/k64_fp16_weights", ops.linear_f16x3(x64, w64.half().float(), b))
    put("linear/k64_acc", ops.linear_f16x3_acc(x64, w64, b, rnd(300, 256).to(dev).contiguous()))
    put("mha/2x77_h2", ops.mha_f16x3(rnd(2, 77, 3 * 128).to(dev), 2))
    put("mha/1x577_h1", ops.mha_f16x3(rnd(1, 577, 3 * 64).to(dev), 1))
    put("conv24/k3_c36_o64", ops.conv24_f16x3(rnd(2, 24, 24, 36).to(dev), rnd(64, 36, 3, 3, s=0.05).to(dev), rnd(64, s=0.1).to(dev), relu=True))
    dec = StandardDecoder("cpu", True, True, input_dim=128, decoder_dims=[64, 32]).eval()
    dec.load_state_dict(orc.analytic_state_dict(dec.state_dict(), seed=7), strict=True)
    n, h, w = 3, 8, 16
    with torch.no_grad():
        lg, fm = HipDecoder(dec.to(dev), dev).forward(rnd(n, 128, h, w).to(dev), rnd(n, 256, 2 * h, 2 * w, s=2.0).to(dev),
                                                      rnd(n, 128, 4 * h, 4 * w, s=0.5).to(dev))
    put("decoder/logits", lg)
    put("decoder/featmap", fm)
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print(f"{len(out)} arrays -> {out_path}")


def time_windows():
    import _devlib  # noqa: F401
    torch, rnd = _inputs()
    from oryon_amd import ops
    dev = torch.device("cuda", 0)
    qk, v = rnd(128, 24, 24, 256, s=2.0).to(dev), rnd(128, 24, 24, 128).to(dev)
    qkv, pad, bias = rnd(32, 96, 96, 384, s=1.5).to(dev), rnd(384, s=0.5).to(dev), rnd(4, 49, 49).to(dev)
    for name, call in (("fusion_window", lambda: ops.fusion_window_attention(qk, v, 4, 12, 6)),
                       ("swin_window", lambda: ops.swin_window_attention_f32(qkv, pad, bias, 4, 3))):
        for _ in range(10):
            call()
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(4):                                       # a backlog, so that the timed calls wait for the GPU and not for the host
                call()
            e0.record()
            for _ in range(10):
                call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 10)
        print(f"{name}: median {sorted(ts)[len(ts) // 2] * 1e3:.1f} us (min {min(ts) * 1e3:.1f})", flush=True)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 0, (a.files, b.files)
    for k in sorted(a.files):
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))
        print(f"{k}: identical {a[k].shape}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "time":
        time_windows()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)

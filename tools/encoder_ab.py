"""A/B of the PointDSC encoder between two builds of the library, one route per shape.

  ORYON_DEVLIB=/path/to/liboryon_hip.so python tools/encoder_ab.py run out.npz    # one library, one process
  python tools/encoder_ab.py compare a.npz b.npz                                   # every array bit for bit

`run` encodes and registers seeded inputs at four shapes (chain, fused with key split, fused image-fed at 4 waves, plain), writes the
valid rows of feat / conf and the poses T, and prints the median time of an encode call per shape."""
import sys

import numpy as np

# name, layers, C, B, n_cap, ragged
SHAPES = (("chain_b64_n512", 12, 128, 64, 512, False),
          ("fused_split_b1_n512", 12, 128, 1, 512, False),
          ("fused_img_w4_b86_n384", 12, 128, 86, 384, True),
          ("plain_l2c32_b4_n128", 2, 32, 4, 128, False))


def run(out_path):
    import _devlib  # noqa: F401
    import torch
    from oracle import oryon_oracle as orc
    from oryon_amd.pointdsc import PointDSC
    dev = torch.device("cuda", 0)
    out = {}
    for name, L, C, B, n_cap, ragged in SHAPES:
        m = PointDSC(in_dim=6, num_layers=L, num_channels=C, num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1)
        m.load_state_dict(orc.analytic_pointdsc_params(L, C, seed=1), strict=True)
        m = m.to(dev).eval()
        g = torch.Generator().manual_seed(11)
        n = torch.randint(11, n_cap + 1, (B,), generator=g) if ragged else torch.full((B,), n_cap - 12)
        if ragged:
            n[0], n[1], n[2], n[3] = n_cap, 11, 64, 129
        src = torch.zeros((B, n_cap, 3))
        tgt = torch.zeros((B, n_cap, 3))
        for b in range(B):
            k = int(n[b])
            src[b, :k] = torch.rand(k, 3, generator=g) * 0.6 - 0.3
            tgt[b, :k] = src[b, :k] + 0.02 * torch.randn(k, 3, generator=g)
        src, tgt, n32 = src.to(dev), tgt.to(dev), n.to(torch.int32).to(dev)
        for _ in range(3):
            feat, conf = m.encode(src, tgt, n32)
        ts = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                feat, conf = m.encode(src, tgt, n32)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 20)
        T = m.register(src, tgt, n32, torch.zeros(B, dtype=torch.int32, device=dev))[0]
        valid = (torch.arange(n_cap, device=dev)[None, :] < n32[:, None])
        out[name + "/feat"] = torch.where(valid[..., None], feat, torch.zeros_like(feat)).cpu().numpy()
        out[name + "/conf"] = torch.where(valid, conf, torch.zeros_like(conf)).cpu().numpy()
        out[name + "/T"] = T.cpu().numpy()
        assert np.isfinite(out[name + "/feat"]).all() and np.abs(out[name + "/feat"]).sum() > 0
        print(f"{name}: encode median {sorted(ts)[len(ts) // 2] * 1e3:.1f} us (min {min(ts) * 1e3:.1f})", flush=True)
    np.savez(out_path, **out)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 3 * len(SHAPES), (a.files, b.files)
    for k in sorted(a.files):
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))
        print(f"{k}: identical {a[k].shape}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)

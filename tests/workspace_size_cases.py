"""Every `*_workspace_bytes` entry, the decoder's offset table and the engine's arena size over a fixed list of shapes: the smallest
accepted one, one whose element counts are not multiples of 64 (every 256-byte round-up is taken) and the workload's.  None of these
entries touches a device.  sizes(L) -> {label: bytes}; tests/golden/workspace_sizes.json holds what the library returned before
the carving code moved onto one Carver (test_cabi_and_host.py::test_every_workspace_size_is_pinned)."""
import ctypes

ICP_MAX_ROWS = 8192
ENGINE_BASE = dict(B=1, C=256, FH=8, FW=8, HA=8, WA=8, HQ=8, WQ=8, layout=0, dist_th=0.25, n_corrs=500, src_sampling=5000, seed=1,
                   round_f16=0, n_slots=6, overlap=2, gather_sets=2, reg_streams=2, reg_lag=0, screen=1, sample_first=0, x3_prefetch=1,
                   stream_roles=0)
ENGINE_VARIANTS = {"base": {}, "sample_first": dict(sample_first=1000), "no_prefetch": dict(x3_prefetch=0),
                   "ransac": dict(solver=1, ransac_max_iter=10000, ransac_match_err=0.01, ransac_fix_percent=0.9999),
                   "two_slots": dict(n_slots=2, gather_sets=1)}


def pointdsc_handle(L, _lib, num_channels: int, num_layers: int):
    h = ctypes.c_void_p()
    cfg = _lib.PointDSCConfig(in_dim=6, num_layers=num_layers, num_channels=num_channels, num_iterations=10, ratio=0.1, inlier_threshold=0.1,
                              sigma_d=0.1, k=40, nms_radius=0.1)
    assert L.oryon_pointdsc_create(ctypes.byref(h), ctypes.byref(cfg)) == 0
    return h


def sizes(L, _lib) -> dict:
    from oryon_amd import ops
    out = {}

    def put(name, args, value):
        out[f"{name}{tuple(args)}"] = int(value)

    handles = {c: pointdsc_handle(L, _lib, c, layers) for c, layers in ((32, 2), (128, 12))}
    try:
        for c, h in handles.items():                        # (1, 128): key-split attention (att_o / att_ml present); (64, 512): one split
            for B, n_cap in ((1, 128), (3, 384), (64, 512)):
                put(f"oryon_pointdsc_workspace_bytes[C={c}]", (B, n_cap), L.oryon_pointdsc_workspace_bytes(h, B, n_cap))
        for tag, cfg in (("default", {}), ("k63_ratio1", dict(k=63, ratio=1.0))):
            c = ops.spectral_config(**cfg)
            for B, n_cap in ((1, 128), (3, 384), (64, 512), (1, 2048)):
                put(f"oryon_spectral_workspace_bytes[{tag}]", (B, n_cap), L.oryon_spectral_workspace_bytes(ctypes.byref(c), B, n_cap))
        for a in ((1, 128, 1), (3, 384, 777), (64, 512, 10000), (1, 2048, 10000)):
            put("oryon_ransac_workspace_bytes", a, L.oryon_ransac_workspace_bytes(*a))
        for a in ((1, 1, 1), (2, 64, 64), (5, 256, 300), (5, 257, 1), (64, 2048, 2048), (3, ICP_MAX_ROWS, ICP_MAX_ROWS), (65535, 3, 3), (3, 777, 5)):
            put("oryon_icp_workspace_bytes", a, L.oryon_icp_workspace_bytes(*a))
        for a in ((1, 1), (2, 64), (5, 256), (5, 257), (64, 2048), (3, ICP_MAX_ROWS), (65535, 3), (3, 777)):
            put("oryon_icp_plane_workspace_bytes", a, L.oryon_icp_plane_workspace_bytes(*a))
        for a in ((1, 8, 8), (3, 777, 1001), (1, 20000, 20000)):
            put("oryon_gt_corrs_workspace_bytes", a, L.oryon_gt_corrs_workspace_bytes(*a))
        for a in ((1, 1, 1, 1), (3, 37, 53, 777), (64, 480, 640, 30000)):             # (B, H, W, max_faces)
            put("oryon_vsd_workspace_bytes", a, L.oryon_vsd_workspace_bytes(*a))
        for a in ((1, 1), (5, 777), (128, 30000)):                                    # (N, max_faces)
            put("oryon_render_depth_workspace_bytes", a, L.oryon_render_depth_workspace_bytes(*a))
        for a in ((1, 1), (3, 7), (64, 8)):                                           # (B, max_syms)
            put("oryon_pose_bop_workspace_bytes", a, L.oryon_pose_bop_workspace_bytes(*a))
        for a in ((1, 1, 0), (3, 777, 1001), (64, 500, 3136)):                        # (B, n_corr, n_pool)
            put("oryon_feature_loss_workspace_bytes", a, L.oryon_feature_loss_workspace_bytes(*a))
        for a in ((1, 1, 1), (3, 37, 777), (64, 256, 500)):                           # (B, C, n_corr)
            put("oryon_feature_loss_grad_workspace_bytes", a, L.oryon_feature_loss_grad_workspace_bytes(*a))
        for a in ((1,), (3,), (128,)):
            put("oryon_rgb_augment_workspace_bytes", a, L.oryon_rgb_augment_workspace_bytes(*a))
        for a in ((1, 24, 24), (3, 24, 24), (128, 24, 24)):
            put("oryon_decoder_workspace_bytes", a, L.oryon_decoder_workspace_bytes(*a))
            off = (ctypes.c_int64 * 3)()
            assert L.oryon_decoder_workspace_layout(*a, off) == 0
            for i in range(3):
                put(f"oryon_decoder_workspace_layout[{i}]", a, off[i])
        for tag, change in ENGINE_VARIANTS.items():
            cfg = _lib.EngineConfig(**dict(ENGINE_BASE, **change))
            put(f"oryon_engine_arena_bytes[{tag}]", (), L.oryon_engine_arena_bytes(ctypes.byref(cfg), handles[128]))
    finally:
        for h in handles.values():
            L.oryon_pointdsc_destroy(h)
    return out

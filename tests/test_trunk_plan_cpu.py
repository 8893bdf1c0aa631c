"""CPU test of evk_trunk_plan (csrc/trunk.hip): the read-only view of the native trunk runner's workspace layout.  It computes nothing and
touches no device memory, so the sizing contract of the runner is checked here, without a GPU: every region inside the workspace, no two
regions overlapping, every offset 256-byte aligned, and the shared buffers (partial statistics rows, split-K slabs, rotating gradient buffers,
column-reduction scratch, the zero vector) at least as large as the `*_bytes` functions of include/evoke_hip.h ask for every pair that
uses them, on whichever route the host-side routing picks."""
import ctypes as C

import pytest

RESNET101 = ((3, 4, 23, 3), (64, 128, 256, 512))
CASES = [
    ('resnet101 64x384x384', RESNET101, 64, 384, 384),
    ('resnet101 3x224x224', RESNET101, 3, 224, 224),
    ('reduced (2,1,2,1) 3x96x160', ((2, 1, 2, 1), (64, 128, 256, 512)), 3, 96, 160),
    ('reduced narrow (1,1,1,1) 5x96x160', ((1, 1, 1, 1), (16, 32, 64, 128)), 5, 96, 160),
    ('reduced (1,1,1,1) 1x32x64', ((1, 1, 1, 1), (64, 128, 256, 512)), 1, 32, 64),
]


def make_cfg(H, blocks, planes, stride=(1, 2, 2, 2), eps=1e-5, momentum=0.1):
    cfg = H.TrunkCfg()
    for i in range(4):
        cfg.blocks[i], cfg.planes[i], cfg.stride[i] = blocks[i], planes[i], stride[i]
    cfg.eps, cfg.momentum = eps, momentum
    return cfg


def regions(pairs, plan):
    """[(name, offset, bytes)] of every region the plan lays out"""
    out = []
    for i, p in enumerate(pairs):
        out += [('pair%d.%s' % (i, n), getattr(p, n), p.act_bytes) for n in ('y', 'z', 'dy')]
        out += [('pair%d.stats' % i, p.stats, p.stats_bytes), ('pair%d.sums' % i, p.sums, p.sums_bytes)]
        if p.wflip >= 0:
            out.append(('pair%d.wflip' % i, p.wflip, p.wflip_bytes))
        if p.wcls >= 0:
            out.append(('pair%d.wcls' % i, p.wcls, p.wcls_bytes))
    for n in ('xpad', 'wp', 'dwp', 'pooled', 'pool_idx', 'red', 'slab', 'zeros', 'part'):
        out.append((n, getattr(plan, n), getattr(plan, n + '_bytes')))
    out += [('gbuf%d' % k, plan.gbuf[k], plan.gbuf_bytes) for k in range(6)]
    return out


@pytest.mark.parametrize('name,arch,N,Hh,Ww', CASES, ids=[c[0].replace(' ', '_') for c in CASES])
def test_trunk_plan_regions_are_disjoint_aligned_and_large_enough(name, arch, N, Hh, Ww):
    from evoke_amd import hip as H
    L = H.lib
    cfg = make_cfg(H, *arch)
    pairs, plan = H.trunk_plan(cfg, N, Hh, Ww)
    total = L.evk_trunk_ws_bytes(C.byref(cfg), N, Hh, Ww)
    assert total > 0 and plan.total == total
    assert plan.n_pairs == len(pairs) == L.evk_trunk_num_pairs(C.byref(cfg)) and plan.n_blocks == sum(arch[0])

    # geometry of the view: the stem, then conv1 / conv2 / conv3 (/ downsample for the first block of a layer) per bottleneck
    assert (pairs[0].role, pairs[0].block, pairs[0].C, pairs[0].M) == (0, -1, 64, N * (Hh // 2) * (Ww // 2))
    roles = [(p.block, p.role) for p in list(pairs)[1:]]
    want_roles, b = [], 0
    for layer in range(4):
        for k in range(arch[0][layer]):
            want_roles += [(b, 1), (b, 2), (b, 3)] + ([(b, 4)] if k == 0 else [])
            b += 1
    assert roles == want_roles
    for p in list(pairs)[1:]:
        g = p.g
        assert p.C == g.Co and p.M == g.N * g.Ho * g.Wo and g.N == N and p.act_bytes == p.M * p.C * 2
        assert g.Ho == (g.Hi + 2 * g.pad_h - g.KH) // g.stride_h + 1 and g.Wo == (g.Wi + 2 * g.pad_w - g.KW) // g.stride_w + 1
        assert p.stats_bytes == 6 * 4 * p.C and p.sums_bytes == 2 * 4 * p.C

    # every region inside [0, total), aligned, and no two of them overlapping
    regs = regions(pairs, plan)
    for rn, off, nb in regs:
        assert off >= 0 and off % 256 == 0, (rn, off)
        assert nb >= 0 and off + nb <= total, (rn, off, nb, total)
    live = sorted((off, off + nb, rn) for rn, off, nb in regs if nb > 0)
    for (a0, a1, an), (b0, b1, bn) in zip(live, live[1:]):
        assert a1 <= b0, 'regions %s [%d, %d) and %s [%d, %d) overlap' % (an, a0, a1, bn, b0, b1)

    # fixed-size regions
    assert plan.xpad_bytes == N * (Hh + 6) * (Ww + 8) * 4 * 2 and plan.wp_bytes == 64 * 224 * 2 and plan.dwp_bytes == 64 * 224 * 4
    assert plan.pooled_bytes == N * (Hh // 4) * (Ww // 4) * 64 * 2 and plan.pool_idx_bytes == N * (Hh // 4) * (Ww // 4) * 64

    # ---- the sizing contract of the shared buffers -------------------------------------------------------------------------------------
    part, slab, gcap = plan.part_bytes, plan.slab_bytes, plan.gbuf_bytes
    # stem: forward statistics rows (tile path and halo kernel), weight-gradient slabs (both routes)
    assert part >= L.evk_conv_stats_bytes(pairs[0].M, 64)
    assert slab >= L.evk_stem_wgrad_ws_bytes(N, Hh, Ww)
    if L.evk_stem_halo_supported(N, Hh, Ww):
        assert part >= L.evk_stem_halo_part_bytes(N, Hh, Ww) and slab >= L.evk_stem_halo_wgrad_ws_bytes(N, Hh, Ww)
    by_block = {}
    for i, p in enumerate(pairs):
        if i:
            by_block.setdefault(p.block, {})[p.role] = p
    for i, p in enumerate(pairs):
        assert gcap >= p.act_bytes, (i, 'a block-level gradient has the shape of a pair output')
        assert plan.red_bytes >= L.evk_colreduce_ws_bytes(p.C) and plan.zeros_bytes >= 4 * p.C, i
        if i == 0:
            continue
        g = p.g
        Min = g.N * g.Hi * g.Wi
        gp = C.byref(g)
        assert gcap >= Min * g.Ci * 2, (i, 'the data gradient of a pair has the shape of its input')
        # forward: partial statistics rows [nblk][2][Co] of whichever kernel takes the convolution
        assert part >= L.evk_conv_stats_bytes(p.M, p.C), i
        if g.KH == 1 and g.stride_h == 1:
            if L.evk_conv1x1_ws_supported(p.M, g.Ci, g.Co):
                assert part >= L.evk_conv1x1_ws_part_bytes(p.M, g.Ci, g.Co), i
            if L.evk_gemm_strip_supported(p.M, g.Co, g.Ci):
                assert part >= L.evk_gemm_strip_part_bytes(p.M, g.Co), i
        if g.KH == 3 and g.stride_h == 1 and L.evk_conv3x3_halo_supported(g.N, g.Hi, g.Wi, g.Ci, g.Co):
            assert part >= L.evk_conv3x3_halo_part_bytes(g.N, g.Hi, g.Wi, g.Co), i
        # backward: split-K slabs of the weight gradient
        assert slab >= L.evk_conv2d_wgrad_ws_bytes(gp), i
        if g.KH == 3 and g.stride_h == 1 and L.evk_conv3x3_wgrad_halo_supported(g.N, g.Hi, g.Wi, g.Ci, g.Co):
            assert slab >= L.evk_conv3x3_wgrad_halo_ws_bytes(g.N, g.Hi, g.Wi, g.Ci, g.Co), i
        # backward: gate statistics [nblk][2][Ci] of the data gradient that feeds the batch norm of this pair's INPUT (conv2, conv3), and the
        # [nblk][3][Ci] rows of the block-input gradient (conv1 of every block)
        if p.role in (2, 3):
            assert part >= L.evk_conv_stats_bytes(Min, g.Ci), i
            if g.KH == 1 and L.evk_conv1x1_ws_supported(Min, g.Co, g.Ci):
                assert part >= L.evk_conv1x1_ws_part_bytes(Min, g.Co, g.Ci), i
            if g.KH == 1 and L.evk_gemm_strip_supported(Min, g.Ci, g.Co):
                assert part >= L.evk_gemm_strip_part_bytes(Min, g.Ci), i
            if g.KH == 3 and g.stride_h == 1 and L.evk_conv3x3_halo_supported(g.N, g.Hi, g.Wi, g.Co, g.Ci):
                assert part >= L.evk_conv3x3_halo_part_bytes(g.N, g.Hi, g.Wi, g.Ci), i
        if p.role == 1:
            assert part >= L.evk_conv_xstat_bytes(gp), i
        # flipped / class weights: one 16-bit copy of the filter
        if p.wflip >= 0:
            assert p.wflip_bytes == g.Co * g.KH * g.KW * g.Ci * 2, i
            assert (g.KH == 3 and g.stride_h == 1) or (g.KH == 1 and g.Co > g.Ci), i
        if p.wcls >= 0:
            assert g.KH == 3 and g.stride_h == 2 and p.wcls_bytes == g.Co * 9 * g.Ci * 2, i
            assert L.evk_conv3x3s2_dgrad_parity_supported(gp) == 1 and gcap >= L.evk_conv3x3s2_dgrad_parity_ws_bytes(gp), i
        elif g.KH == 3 and g.stride_h == 2 and L.evk_conv3x3s2_dgrad_parity_supported(gp) == 1:
            assert gcap < L.evk_conv3x3s2_dgrad_parity_ws_bytes(gp), (i, 'parity route dropped although its scratch fits')
        if p.role == 4 and g.stride_h == 2:             # compact shortcut gradient: the product on a quarter of the rows
            assert gcap >= g.N * g.Ho * g.Wo * g.Ci * 2, i


def test_trunk_plan_refuses_bad_arguments_on_the_host():
    from evoke_amd import hip as H
    L = H.lib
    cfg = make_cfg(H, *RESNET101)
    n = L.evk_trunk_num_pairs(C.byref(cfg))
    pairs, plan = (H.TrunkPairView * n)(), H.TrunkPlanView()
    assert L.evk_trunk_plan(C.byref(cfg), 2, 100, 96, pairs, n, C.byref(plan)) != 0 and b'multiple of 32' in L.evk_last_error()
    assert L.evk_trunk_plan(C.byref(cfg), 2, 96, 96, pairs, n - 1, C.byref(plan)) != 0 and b'pairs' in L.evk_last_error()
    assert L.evk_trunk_plan(C.byref(cfg), 2, 96, 96, None, n, C.byref(plan)) != 0
    bad = make_cfg(H, (1, 1, 1, 1), (64, 96, 256, 512))          # planes must be a power of two
    assert L.evk_trunk_plan(C.byref(bad), 2, 96, 96, pairs, 17, C.byref(plan)) != 0 and b'bad layer' in L.evk_last_error()
    assert L.evk_trunk_ws_bytes(C.byref(bad), 2, 96, 96) == -1

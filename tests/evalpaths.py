"""The launcher arithmetic of the eval-mode gradient calls (siggan_g_latent_objective_grad, siggan_g_param_grad) restated in
plain Python: which implicit-GEMM tile launch_gconv picks and how it splits K, how launch_fc_dz / k_obj_fin_tiles /
launch_bn_eval_bwd cut a batch into workgroups.  No torch, no GPU: test_eval_paths_cpu.py holds the restatement to the constants
in the sources and to the path each case of objectivecommon.BATCH_CASES exists for; test_eval_grad_batches_gpu.py holds the
library's per-launch profile to it.  A retuned threshold then shows up as a changed case list, not as silently lost coverage."""

# ---- the constants restated (test_eval_paths_cpu.py reads them back from the sources) ------------------------------------------
G_CHAIN = {64: (256, 128, 64, 32, 32), 128: (512, 256, 128, 64, 32, 32)}      # siggan.hip build_layout: gC[0 .. Lg]
D_CHAIN = {64: (1, 64, 128, 256, 512), 128: (1, 64, 128, 256, 512, 512)}      # dC[0 .. Ld]
BK = 32                          # gconv_parts.h: the K-tile
SPLIT_BELOW = 384                # gconv.hip launch_gconv: fewer workgroups than this split K
SPLIT_FILL = 512                 # ... into ceil(512 / workgroups) parts, at most nk / 4 and at most MAX_SLABS
MAX_SLABS = 8
T128_FROM = 512                  # 128x128 tiles only where they still give this many workgroups
SLAB_K_FLOATS = 16 << 20         # siggan.hip: slab_k_floats
PARTIAL_FLOATS = 2 << 20         # ctx.h
PARTIAL_RESERVED = 64            # eval.hip: the last 64 floats of `partial` are siggan_op_adam's scratch slot
DZ_BT, DZ_SUB = 8, 64            # latent.hip: images per k_fc_dz workgroup, features per staged chunk
OBJ_IMAGES = 4                   # latent.hip k_obj_fin_tiles: one wave per image, four per workgroup
BN_EVAL_ROWS = 512               # paramgrad.hip launch_bn_eval_bwd: rows per workgroup before the carve forces more


def cdiv(a, b):
    return (a + b - 1) // b


def gconv_plan(form, M, Ci, Co):
    """launch_gconv on an fp32 context without a classifier rider and with a slab: (kernel, slabs, kq) -- `slabs` > 1: that
    many K slabs and the epilogue in k_splitk_epilogue; kq 2: the in-workgroup two-way K split (one launch, no slabs)."""
    ncls = 1 if form == 0 else 4
    blocks = lambda bm, bn: cdiv(M, bm) * (Co // bn) * ncls
    nk = (16 if form == 0 else 4) * (Ci // BK)
    out_floats = M * Co * (1 if form == 0 else 4)

    def splits(nblk):
        ns = 1
        if nblk < SPLIT_BELOW:
            ns = min(cdiv(SPLIT_FILL, nblk), nk // 4, MAX_SLABS)
            if ns > 1 and ns * out_floats > SLAB_K_FLOATS:
                ns = SLAB_K_FLOATS // out_floats
            ns = max(ns, 1)
        return ns

    if Co >= 64:
        if Co >= 128 and blocks(128, 128) >= T128_FROM:
            return ("k_gconv<128,128>", 1, 1)
        ns = splits(blocks(64, 64))
        if ns == 2 and nk % 2 == 0:
            return ("k_gconv<64,64>", 1, 2)
        return ("k_gconv<64,64>", ns, 1)
    return ("k_gconv<128,32>", splits(blocks(128, 32)), 1)


def g_chain(size, batch, table=True):
    """The Generator's eval-mode input-gradient GEMMs, l = Lg .. 1 (eval.hip latent_objective_grad / param_grad): form 0, rows of
    the small side, EPI_LRELU_BWD on the stored activation for l >= 2 (`table`: with the per-image scale table lg_tab), raw into
    block 0.  [{l, kernel, form, epi, M, Ci, Co, slabs, kq}]"""
    gc = G_CHAIN[size]
    out = []
    for l in range(len(gc) - 1, 0, -1):
        h = 4 << (l - 1)
        M, Ci, Co = batch * h * h, gc[l], gc[l - 1]
        kernel, slabs, kq = gconv_plan(0, M, Ci, Co)
        out.append(dict(l=l, kernel=kernel, form=0, epi="lrelu_bwd" if l >= 2 else "raw", M=M, Ci=Ci, Co=Co, slabs=slabs, kq=kq))
    return out


def d_chain(size, batch):
    """The Discriminator's eval-mode input-gradient chain, l = Ld .. 2 (passes.hip objective_seeds): form 1, EPI_LRELU_BWD
    without a table."""
    dc = D_CHAIN[size]
    out = []
    for l in range(len(dc) - 1, 1, -1):
        h = size >> l
        M, Ci, Co = batch * h * h, dc[l], dc[l - 1]
        kernel, slabs, kq = gconv_plan(1, M, Ci, Co)
        out.append(dict(l=l, kernel=kernel, form=1, epi="lrelu_bwd", M=M, Ci=Ci, Co=Co, slabs=slabs, kq=kq))
    return out


def fc_dz_plan(size, latent, batch):
    """launch_fc_dz: nsplit workgroups along the features (halved while the partial sums outgrow the carve), image tiles of
    DZ_BT, the live rows of the last tile, 64-feature chunks per workgroup (more than one: the f0 loop), passes over k."""
    F = G_CHAIN[size][0] * 16
    nsplit = F // DZ_SUB
    while nsplit > 1 and nsplit * batch * latent > PARTIAL_FLOATS - PARTIAL_RESERVED:
        nsplit >>= 1
    return dict(nsplit=nsplit, tiles=cdiv(batch, DZ_BT), last_rows=(batch - 1) % DZ_BT + 1, chunks=F // nsplit // DZ_SUB,
                k_passes=cdiv(latent, 64), fused_fc=latent % 4 == 0)


def obj_fin_plan(size, batch):
    """launch_obj_fin_tiles: objective workgroups (four waves = four images; the live waves of the last) and, per scale table of
    blocks 1 .. Lg - 1, the copy workgroups of 256 float4."""
    gc = G_CHAIN[size]
    return dict(blocks=cdiv(batch, OBJ_IMAGES), last_waves=(batch - 1) % OBJ_IMAGES + 1,
                tile_blocks=[cdiv(batch * (gc[l] // 4), 256) for l in range(1, len(gc) - 1)])


def bn_eval_plan(size, batch):
    """launch_bn_eval_bwd per block l = 1 .. Lg: (workgroups, rows of the last one)."""
    gc = G_CHAIN[size]
    out = []
    for l in range(1, len(gc)):
        h = 4 << l
        R, rows = batch * h * h, BN_EVAL_ROWS
        while cdiv(R, rows) * 2 * gc[l] > PARTIAL_FLOATS - PARTIAL_RESERVED:
            rows *= 2
        out.append((cdiv(R, rows), (R - 1) % rows + 1))
    return out


def describe(size, latent, batch):
    return dict(g=g_chain(size, batch), d=d_chain(size, batch), fc_dz=fc_dz_plan(size, latent, batch),
                obj=obj_fin_plan(size, batch), bn_eval=bn_eval_plan(size, batch))


if __name__ == "__main__":
    for case in [(64, 100, 1), (64, 100, 2), (64, 100, 3), (128, 128, 2), (64, 100, 9), (64, 50, 13), (64, 100, 64), (128, 128, 12),
                 (64, 100, 256)]:
        print(case)
        for k, v in describe(*case).items():
            if isinstance(v, list) and v and isinstance(v[0], dict):
                for e in v:
                    print("   ", k, e)
            else:
                print("   ", k, v)

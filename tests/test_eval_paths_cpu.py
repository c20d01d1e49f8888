"""evalpaths.py -- the launcher arithmetic of the eval-mode gradient calls restated in Python -- held to the constants in the
sources it restates and to the paths each case of objectivecommon.BATCH_CASES exists for.  A retuned threshold (PARTIAL_FLOATS,
DZ_BT, the 384 / 512 workgroup counts of launch_gconv, the channel chains) fails here and names the case that no longer reaches
its path, instead of the coverage going quietly.  The GPU side, test_eval_grad_batches_gpu.py, holds the library's own launch
profile to the same restatement."""
import os
import re

import evalpaths as E
from common import O, ROOT
from objectivecommon import BATCH_CASES, CASES

CSRC = os.path.join(ROOT, "signature-gan_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def ints(s):
    return tuple(int(x) for x in s.split(","))


def test_the_restated_constants_are_the_sources():
    ctx, latent, gconv, parts = src("ctx.h"), src("latent.hip"), src("gconv.hip"), src("gconv_parts.h")
    siggan, eval_, pgrad = src("siggan.hip"), src("eval.hip"), src("paramgrad.hip")
    assert int(one(r"PARTIAL_FLOATS = \(int64_t\)(\d+) << 20;", ctx)) << 20 == E.PARTIAL_FLOATS
    assert eval_.count("PARTIAL_FLOATS - 64") == 2 and E.PARTIAL_RESERVED == 64          # launch_fc_dz's and launch_bn_eval_bwd's caps
    assert ints(",".join(one(r"constexpr int DZ_BT = (\d+), DZ_SUB = (\d+);", latent))) == (E.DZ_BT, E.DZ_SUB)
    assert "int nsplit = F / DZ_SUB;" in latent and "nsplit >>= 1" in latent
    assert "b = bid * 4 + (threadIdx.x >> 6)" in latent and "const int nbl = cdiv(B, 4);" in latent and E.OBJ_IMAGES == 4
    assert "cdiv((int64_t)B * (t.C[i] / 4), 256)" in latent
    assert int(one(r"static constexpr int BK = (\d+);", parts)) == E.BK
    assert int(one(r"if \(a\.slab && nblk < (\d+)\)", gconv)) == E.SPLIT_BELOW
    assert int(one(r"ns = \((\d+) \+ nblk - 1\) / nblk;", gconv)) == E.SPLIT_FILL
    assert "if (ns > nk / 4) ns = nk / 4;" in gconv
    assert int(one(r"if \(ns > (\d+)\) ns = \d+;", gconv)) == E.MAX_SLABS
    assert int(one(r"blocks\(128, 128\) >= (\d+)\)", gconv)) == E.T128_FROM
    assert int(one(r"slab_k_floats = \(int64_t\)(\d+) << 20;", siggan)) << 20 == E.SLAB_K_FLOATS
    g64, g128 = one(r"g64\[\] = \{([\d, ]+)\}, g128\[\] = \{([\d, ]+)\}", siggan)
    d64, d128 = one(r"d64\[\] = \{([\d, ]+)\}, d128\[\] = \{([\d, ]+)\}", siggan)
    assert {64: ints(g64), 128: ints(g128)} == E.G_CHAIN == dict(O.G_CHAIN)
    assert {64: ints(d64), 128: ints(d128)} == E.D_CHAIN and {s: c[1:] for s, c in E.D_CHAIN.items()} == dict(O.D_CHAIN)
    assert int(one(r"int64_t rows = (\d+);", pgrad)) == E.BN_EVAL_ROWS


# What each batch case exists for, written out: the Generator chain's (l, kernel, rows M, slabs, kq) for the blocks that run
# EPI_LRELU_BWD with the scale table, the Discriminator chain's, and the workgroup arithmetic of the small kernels.
_S, _M, _N = "k_gconv<64,64>", "k_gconv<128,32>", "k_gconv<128,128>"
WANT = {
    (64, 100, 9): dict(
        g=[(4, _M, 9 * 1024, 4, 1), (3, _S, 9 * 256, 4, 1), (2, _S, 9 * 64, 8, 1)],          # 72 / 36 / 18 workgroups: all slab-split
        d=[(4, _S, 9 * 16, 8, 1), (3, _S, 9 * 64, 8, 1), (2, _S, 9 * 256, 4, 1)],
        fc_dz=dict(nsplit=64, tiles=2, last_rows=1, chunks=1, k_passes=2, fused_fc=True),
        obj=dict(blocks=3, last_waves=1, tile_blocks=[2, 1, 1]), bn_block1=(2, 64)),
    (64, 50, 13): dict(
        g=[(4, _M, 13 * 1024, 4, 1), (3, _S, 13 * 256, 4, 1), (2, _S, 13 * 64, 8, 1)],
        d=[(4, _S, 13 * 16, 8, 1), (3, _S, 13 * 64, 5, 1), (2, _S, 13 * 256, 3, 1)],         # 104 / 208 workgroups: ceil(512 / .)
        fc_dz=dict(nsplit=64, tiles=2, last_rows=5, chunks=1, k_passes=1, fused_fc=False),
        obj=dict(blocks=4, last_waves=1, tile_blocks=[2, 1, 1]), bn_block1=(2, 320)),
    (64, 100, 64): dict(
        g=[(4, _M, 64 * 1024, 1, 1),             # 512 workgroups: unsplit, epilogue and table in k_gconv<128,32>
           (3, _S, 64 * 256, 1, 2),              # 256 workgroups -> two-way: the two-quad kernel
           (2, _S, 64 * 64, 4, 1)],              # 128 workgroups -> four slabs
        d=[(4, _S, 64 * 16, 1, 2), (3, _S, 64 * 64, 1, 1), (2, _S, 64 * 256, 1, 1)],          # 256 / 512 / 1024 workgroups
        fc_dz=dict(nsplit=64, tiles=8, last_rows=8, chunks=1, k_passes=2, fused_fc=True),
        obj=dict(blocks=16, last_waves=4, tile_blocks=[8, 4, 2]), bn_block1=(8, 512)),
    (128, 128, 12): dict(
        g=[(5, _M, 12 * 4096, 1, 1),             # exactly 384 workgroups: the first batch that is not split
           (4, _S, 12 * 1024, 3, 1),             # 192 workgroups -> ceil(512 / 192) = 3 slabs
           (3, _S, 12 * 256, 6, 1), (2, _S, 12 * 64, 8, 1)],
        d=[(5, _S, 12 * 16, 6, 1), (4, _S, 12 * 64, 3, 1), (3, _S, 12 * 256, 1, 1), (2, _S, 12 * 1024, 1, 1)],
        fc_dz=dict(nsplit=128, tiles=2, last_rows=4, chunks=1, k_passes=2, fused_fc=True),
        obj=dict(blocks=3, last_waves=4, tile_blocks=[3, 2, 1, 1]), bn_block1=(2, 256)),
    (64, 100, 256): dict(
        g=[(4, _M, 256 * 1024, 1, 1), (3, _S, 256 * 256, 1, 1), (2, _S, 256 * 64, 1, 1)],     # 2048 / 1024 / 512 workgroups
        d=[(4, _S, 256 * 16, 1, 1), (3, _N, 256 * 64, 1, 1), (2, _S, 256 * 256, 1, 1)],       # l = 3: 512 tiles of 128x128
        fc_dz=dict(nsplit=64, tiles=32, last_rows=8, chunks=1, k_passes=2, fused_fc=True),
        obj=dict(blocks=64, last_waves=4, tile_blocks=[32, 16, 8]), bn_block1=(32, 512)),
    (64, 512, 64): dict(                          # the GEMMs of (64, 100, 64): they do not see the latent
        g=[(4, _M, 64 * 1024, 1, 1), (3, _S, 64 * 256, 1, 2), (2, _S, 64 * 64, 4, 1)],
        d=[(4, _S, 64 * 16, 1, 2), (3, _S, 64 * 64, 1, 1), (2, _S, 64 * 256, 1, 1)],
        # 64 * 64 * 512 = 2097152 > 2097088: nsplit halved once, two 64-feature chunks per k_fc_dz workgroup (the f0 loop)
        fc_dz=dict(nsplit=32, tiles=8, last_rows=8, chunks=2, k_passes=8, fused_fc=True),
        obj=dict(blocks=16, last_waves=4, tile_blocks=[8, 4, 2]), bn_block1=(8, 512)),
}


def test_every_batch_case_reaches_what_it_exists_for():
    assert [c[:3] for c, _ in BATCH_CASES] == list(WANT)
    for (size, latent, batch, slope, sn), _ in BATCH_CASES:
        got, want = E.describe(size, latent, batch), WANT[(size, latent, batch)]
        tup = lambda chain, epi: [(e["l"], e["kernel"], e["M"], e["slabs"], e["kq"]) for e in chain if e["epi"] == epi]
        assert tup(got["g"], "lrelu_bwd") == want["g"], (batch, tup(got["g"], "lrelu_bwd"))
        assert tup(got["d"], "lrelu_bwd") == want["d"], (batch, tup(got["d"], "lrelu_bwd"))
        assert got["fc_dz"] == want["fc_dz"] and got["obj"] == want["obj"] and got["bn_eval"][0] == want["bn_block1"], (batch, got)


def test_the_small_parity_cases_reach_none_of_it():
    """Why the batch cases exist: at B <= 3 (objectivecommon.CASES) every EPI_LRELU_BWD GEMM of both chains is slab-split (its
    epilogue runs in k_splitk_epilogue), k_fc_dz has one image tile, the objective one workgroup, every table copy one
    workgroup, and k_bn_eval_bwd's first block one chunk."""
    for size, latent, batch, slope, sn in CASES:
        got = E.describe(size, latent, batch)
        assert all(e["slabs"] > 1 and e["kq"] == 1 for e in got["g"] + got["d"]), (size, batch)
        assert got["fc_dz"]["tiles"] == 1 and got["obj"]["blocks"] == 1 and set(got["obj"]["tile_blocks"]) == {1}
        assert got["bn_eval"][0][0] == 1


def test_where_the_fc_dz_chunk_walk_begins_and_what_no_allowed_batch_reaches():
    """k_fc_dz's walk over several 64-feature chunks needs nsplit halved, i.e. nsplit * B * latent beyond the carve: B * latent
    > 32767 at 64x64 -- B >= 328 at latent 100, B = 256 from latent 128, B = 64 from latent 512 (the batch case that runs it)
    -- and B * latent > 16383 at 128x128.  Stated so that it is not mistaken for covered: the Generator chain's k_gconv<128,128>
    (form 0, EPI_LRELU_BWD with a table) needs 512 tiles of 128 rows at 128 output channels, B >= 1023 at 64x64; the batch
    cases stop at 256."""
    assert E.fc_dz_plan(64, 100, 327)["chunks"] == 1 and E.fc_dz_plan(64, 100, 328)["chunks"] == 2
    assert E.fc_dz_plan(64, 127, 256)["chunks"] == 1 and E.fc_dz_plan(64, 128, 256)["chunks"] == 2
    assert E.fc_dz_plan(64, 511, 64)["chunks"] == 1 and E.fc_dz_plan(64, 512, 64)["chunks"] == 2
    assert E.fc_dz_plan(128, 128, 127)["chunks"] == 1 and E.fc_dz_plan(128, 128, 128)["chunks"] == 2
    assert [E.fc_dz_plan(*c[:3])["chunks"] for c, _ in BATCH_CASES] == [1, 1, 1, 1, 1, 2]
    assert all(e["kernel"] != _N for b in (256, 1022) for e in E.g_chain(64, b))
    assert [e["kernel"] for e in E.g_chain(64, 1023) if e["l"] == 2] == [_N]

"""Bit-for-bit comparison of two builds of the library over everything the derived-state tables feed.

    python profiles/derived_tables_bitwise.py --parent PARENT.so [--new NEW.so] [--also NAME=OTHER.so] [--set small|tiles|both]
                                              [--brief] [--out FILE.json]

Each build runs in a fresh process of its own (the library is loaded once per process, through SIGGAN_LIB_PATH).  For every
seeded configuration below: three train_steps (clipping on the second, the next real batch staged, z and dropout from the
library RNG), then an eval g_forward, a d_forward, one g_latent_objective_grad, a g_generate_u8 with stroke counters, a
d_score_u8, a seeded g_latent_objective_grad, two g_param_grads (first_layer 0 and a middle one) and one g_compute_grads.
Recorded: the sha256 of every arena (params, grads, both moments, step counts), the BatchNorm running statistics and counters,
the spectral-norm u / v, every step's metrics buffer and every call's outputs.  A call a context refuses (the latent objective on a 16-bit one) is
recorded by its message, which must be equal too.  --also: further builds held to the same hashes; what they print to
stderr behind the prefix TABLECMP is kept in the result (a scratch build that compares its job tables with the parent's
builders reports there).

--set: `small` (the default) is the nine small-batch configurations, whose conv GEMMs go through the split-K slabs, the
k_splitk_epilogue tail and the KQ = 2 kernels; `tiles` is the batches at which the epilogues run inside the GEMM kernels and
the larger tiles are chosen, with the LeakyReLU Generator for the LK instantiations.  With `tiles` or `both`, every
configuration also records the distinct GEMM launches of one profiled step on an engine of its own (Engine.prof_launches;
profiling turns the riders off), and the result says which epilogue ran which way -- inside a GEMM kernel, inside a KQ = 2
kernel, through k_splitk_epilogue -- for fp32 and for the 16-bit types; a combination no shape selects is listed with the
launcher condition it needs."""
import argparse, hashlib, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name, Engine arguments, batch, extras
CONFIGS = [
    ("f32_s64_b4", dict(dtype="f32", image_size=64, latent_dim=100), 4, {}),
    ("f32_s64_b5", dict(dtype="f32", image_size=64, latent_dim=100), 5, {}),                 # 80 riders: an odd count
    ("f32_s128_z128_b4", dict(dtype="f32", image_size=128, latent_dim=128), 4, {}),
    ("bf16_s64_b4", dict(dtype="bf16", image_size=64, latent_dim=100), 4, {}),               # packed update, separate first block
    ("f16_s64_b4", dict(dtype="f16", image_size=64, latent_dim=100), 4, {}),                 # two-launch update, k_prepare every step
    ("f32_s64_z50_b8", dict(dtype="f32", image_size=64, latent_dim=50), 8, {}),              # generic fc: k-major copy, no packed G update
    ("f32_s64_b4_sn", dict(dtype="f32", image_size=64, latent_dim=100, spectral_norm=True), 4, {}),
    ("f32_s64_b4_ablation_leaky", dict(dtype="f32", image_size=64, latent_dim=100, g_activation="leaky_relu"), 4, {"ablation": True}),
    ("f32_s64_b4_graph", dict(dtype="f32", image_size=64, latent_dim=100), 4, {"graph": True}),
]

TILE_CONFIGS = [
    ("f32_s64_b64", dict(dtype="f32", image_size=64, latent_dim=100), 64, {}),
    ("bf16_s64_b64", dict(dtype="bf16", image_size=64, latent_dim=100), 64, {}),
    ("f16_s128_z128_b32", dict(dtype="f16", image_size=128, latent_dim=128), 32, {}),
    ("f32_s128_z128_b32", dict(dtype="f32", image_size=128, latent_dim=128), 32, {}),
    ("f32_s64_b255", dict(dtype="f32", image_size=64, latent_dim=100), 255, {}),             # the 128x128 tile on ragged rows
    ("bf16_s64_b256", dict(dtype="bf16", image_size=64, latent_dim=100), 256, {}),
    ("f32_s64_b64_ablation_leaky", dict(dtype="f32", image_size=64, latent_dim=100, g_activation="leaky_relu"), 64, {"ablation": True}),
    ("bf16_s64_b64_ablation_leaky", dict(dtype="bf16", image_size=64, latent_dim=100, g_activation="leaky_relu"), 64, {"ablation": True}),
]
SETS = {"small": CONFIGS, "tiles": TILE_CONFIGS, "both": CONFIGS + TILE_CONFIGS}
EPIS = ("bias_lrelu_drop", "affine_relu", "lrelu_bwd", "bn_bwd_stats")
WAYS = {
    "gemm": "inside a GEMM kernel: launch_gconv's splits() gives 1 (384 or more workgroups, fewer than 8 K-tiles, or no slab), or the "
            "128x128 tile is taken (Co >= 128 and 512 or more such tiles)",
    "kq2": "inside a KQ = 2 kernel: Co >= 64, the 128x128 tile is not taken, splits(blocks(64, 64)) == 2 (16-bit without the "
           "classifier rider: or 4) and an even number of K-tiles",
    "splitk": "through k_splitk_epilogue: fewer than 384 workgroups and min(ceil(512 / workgroups), K-tiles / 4, 8) slabs, at least 2 "
              "and not taken by KQ = 2; the statistics epilogue also needs 256 % (Co / 4) == 0",
}


def launch_way(l, dtype):
    """Which way a recorded conv GEMM launch ran its epilogue: launch_gconv's tile and split rule (gconv.hip) applied to the
    recorded kernel, form, M, Ci, Co.  The slabs are taken to fit, and the classifier rider is off (profiling turns it off)."""
    tile = {"k_gconv<128,128>": None, "k_gconv<64,64>": (64, 64), "k_gconv<128,32>": (128, 32)}.get(l["kernel"], 0)
    if tile == 0:
        return None                                   # k_gconv_up4, k_wgrad: no split
    if tile is None:
        return "gemm"
    ncls, ntaps = (1, 16) if l["form"] == 0 else (4, 4)
    nk = ntaps * (l["Ci"] // 32)
    nblk = -(-l["M"] // tile[0]) * (l["Co"] // tile[1]) * ncls
    ns = max(1, min(-(-512 // nblk), nk // 4, 8)) if nblk < 384 else 1
    if tile == (64, 64) and nk % 2 == 0 and (ns == 2 or (ns == 4 and dtype != "f32")):
        return "kq2"
    if ns > 1 and l["epi"] == "bn_bwd_stats" and 256 % (l["Co"] // 4) != 0:
        ns = 1
    return "gemm" if ns == 1 else "splitk"


def one_step(eng, extra, real, next_real, B, clip=None):
    if extra.get("ablation"):
        eng.d_compute_grads(real, mask_passes=3)
        eng.d_apply(clip=clip)
        eng.g_compute_grads(B)
        eng.g_apply(clip=clip)
    else:
        eng.train_step(real, clip=clip, next_real=next_real)


def child(out_path, which):
    import torch
    sys.path.insert(0, ROOT)
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd.engine import Engine

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    res = {}
    launches = res["__launches__"] = {}
    for name, kw, B, extra in SETS[which]:
        r = res[name] = {}
        size, latent = kw["image_size"], kw["latent_dim"]
        eng = Engine(max_batch=B, device="cuda:0", seed=7, **kw)
        eng.init_reference(3)
        if extra.get("graph"):
            eng.set_mode(graph=True)
        if extra.get("ablation"):
            eng.set_step_variant("ablation")
        gen = torch.Generator().manual_seed(11)
        reals = [(torch.rand(B, 1, size, size, generator=gen) * 2 - 1).cuda() for _ in range(4)]
        z = torch.randn(B, latent, generator=gen).cuda()
        for i in range(3):
            one_step(eng, extra, reals[i], reals[i + 1], B, clip=1.0 if i == 1 else None)
            torch.cuda.synchronize()
            r[f"step{i}/metrics"] = sha(eng.metrics)
        flat = lambda ts: torch.cat([t.reshape(-1).float() for t in ts])     # (bytes and stroke counters are exact in fp32)
        u8 = (reals[2] * 127.5 + 127.5).clamp(0, 255).to(torch.uint8)[:, 0].contiguous()
        calls = {
            "g_forward": lambda: eng.g_forward(z, training=False),
            "d_forward": lambda: eng.d_forward(reals[3], training=False),
            "g_latent_objective_grad": lambda: flat(eng.g_latent_objective_grad(
                z, target=reals[3], recon_weight=1.0, realism_weight=0.5, prior_weight=0.25, want_terms=True, want_probs=True)),
            "g_generate_u8": lambda: flat(eng.g_generate_u8(z, threshold=0.0)),
            "d_score_u8": lambda: eng.d_score_u8(u8),
            "g_latent_objective_grad_seeded": lambda: flat(eng.g_latent_objective_grad(
                z, target=reals[3], recon_weight=1.0, realism_weight=0.5, prior_weight=0.25, want_terms=True, image_grad=reals[1])),
            "g_param_grad/0": lambda: flat(eng.g_param_grad(z, target=reals[3], realism_weight=0.5, want_terms=True, want_probs=True)),
            "g_param_grad/mid": lambda: flat(eng.g_param_grad(z, target=reals[3], realism_weight=0.5, first_layer=(eng.g_layers + 1) // 2)),
        }
        for cname, fn in calls.items():
            try:
                r[cname] = sha(fn())
            except Exception as e:                                   # refused by this kind of context: the message is the result
                r[cname] = "refused: " + str(e)
        if extra.get("ablation"):                                    # this variant's g_grads belongs to a D half
            eng.d_compute_grads(reals[3], mask_passes=3)
            eng.d_apply()
        eng.g_compute_grads(B)
        torch.cuda.synchronize()
        r["g_compute_grads/metrics"] = sha(eng.metrics)
        for w in "gd":
            for a in ("params", "grads", "exp_avg", "exp_avg_sq", "adam_steps"):
                r[f"{w}_{a}"] = sha(getattr(eng, f"{w}_{a}"))
        for a in ("g_bn_mean", "g_bn_var", "g_bn_batches"):
            r[a] = sha(getattr(eng, a))
        if eng.spectral_norm:
            r["d_sn_u"], r["d_sn_v"] = sha(eng.d_sn_u), sha(eng.d_sn_v)
        eng.close()
        if which != "small":
            # one profiled step and the eval forward on an engine of its own: profiling is process-wide and turns the riders off
            eng = Engine(max_batch=B, device="cuda:0", seed=7, **kw)
            eng.init_reference(3)
            if extra.get("ablation"):
                eng.set_step_variant("ablation")
            eng.prof_enable(True)
            try:
                one_step(eng, extra, reals[0], reals[1], B)
                eng.g_forward(z, training=False)
                torch.cuda.synchronize()
                rows = eng.prof_launches()
            finally:
                eng.prof_enable(False)
                eng.close()
            launches[name] = sorted({json.dumps(l, sort_keys=True) for l in rows})
    with open(out_path, "w") as f:
        json.dump(res, f)


def coverage(launches, which):
    """The distinct launches per configuration with the way each ran its epilogue, and per precision class the ways every
    non-raw epilogue was seen to run."""
    dtypes = {name: kw["dtype"] for name, kw, _, _ in SETS[which]}
    per_cfg, seen, kernels = {}, {"f32": {}, "16-bit": {}}, {"f32": set(), "16-bit": set()}
    for name, rows in launches.items():
        cls = "f32" if dtypes[name] == "f32" else "16-bit"
        per_cfg[name] = []
        for l in map(json.loads, rows):
            kernels[cls].add(l["kernel"])
            if l["M"] < 0:
                per_cfg[name].append(l)
                continue
            way = launch_way(l, dtypes[name])
            per_cfg[name].append(dict(l, way=way))
            if way and l["epi"] in EPIS:
                seen[cls].setdefault(l["epi"] + "/" + way, []).append(f"{name}: {l['kernel']} form {l['form']} M {l['M']} Ci {l['Ci']} Co {l['Co']}")
    table, unreachable = {}, []
    for cls in seen:
        for e in EPIS:
            for w in WAYS:
                hits = seen[cls].get(e + "/" + w, [])
                table[f"{cls}/{e}/{w}"] = hits[:3]
                if not hits:
                    unreachable.append({"precision": cls, "epilogue": e, "way": w, "needs": WAYS[w],
                                        "ran_instead": sorted({k.split("/")[1] for k in seen[cls] if k.startswith(e + "/")})})
    return {"how": launch_way.__doc__, "ways_seen": table, "unreachable_at_these_shapes": unreachable,
            "kernels_seen": {c: sorted(k) for c, k in kernels.items()}, "launches": per_cfg}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new", default=os.path.join(ROOT, "signature-gan_amd", "libsiggan_hip.so"))
    ap.add_argument("--also", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived_tables_bitwise.json"))
    ap.add_argument("--set", default="small", choices=sorted(SETS))
    ap.add_argument("--brief", action="store_true", help="write one sha256 per configuration (over its values in key order) and "
                    "the refusals' messages instead of every hash, and leave the epilogue coverage out: for a change that touches no kernel")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.set)
    builds = [("parent", a.parent), ("new", a.new)] + [tuple(s.split("=", 1)) for s in a.also]
    got, notes, launched = {}, {}, {}
    for name, path in builds:
        tmp = a.out + "." + name + ".tmp"
        env = dict(os.environ, SIGGAN_LIB_PATH=os.path.abspath(path))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp, "--set", a.set], env=env, capture_output=True, text=True,
                           timeout=540)
        if p.returncode != 0:
            print(name, "FAILED", p.returncode, p.stderr[-2000:], flush=True)
            return 1
        got[name] = json.load(open(tmp))
        launched[name] = got[name].pop("__launches__")
        os.remove(tmp)
        lines = [ln for ln in p.stderr.splitlines() if ln.startswith("TABLECMP")]
        if lines:
            notes[name] = sorted(set(lines))
    different = [f"{b}/{c}/{k}" for b in got if b != "parent" for c in got["parent"] for k in got["parent"][c]
                 if got[b][c].get(k) != got["parent"][c][k]]
    result = {
        "what": "seeded training steps and eval calls per configuration, the parent commit's library against this commit's, "
                "sha256 of every arena, buffer, metrics vector and output compared",
        "builds": [b for b, _ in builds],
        "values_per_build": sum(len(v) for v in got["parent"].values()),
        "all_equal": not different,
        "different": different,
        "stderr_notes": notes,
        "table_check": ("done: a scratch build with the parent's table builders beside the new ones compared (memcmp) every PrepTable / "
                        "ApTable and packed-update flag it built in these runs; its counts are in stderr_notes") if notes else "not run",
        "sha256": got["parent"] if not different else got,
    }
    if a.set != "small":
        result["configuration_set"] = a.set
        result["launches_equal"] = all(launched[b] == launched["parent"] for b in launched)
        result["epilogue_coverage"] = cov = coverage(launched["new"], a.set)
        different += [] if result["launches_equal"] else ["launches"]
        result["all_equal"] = not different
    if a.brief and not different:
        result.pop("epilogue_coverage", None)
        result["sha256"] = {c: {"values": len(v), "sha256_of_values": hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest(),
                                "refused": {k: s for k, s in v.items() if s.startswith("refused")}} for c, v in got["parent"].items()}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ("builds", "values_per_build", "all_equal", "different", "stderr_notes")}), flush=True)
    if a.set != "small":
        print(json.dumps({"launches_equal": result["launches_equal"], "unreachable": cov["unreachable_at_these_shapes"],
                          "kernels_seen": cov["kernels_seen"]}), flush=True)
    return 0 if not different else 1


if __name__ == "__main__":
    sys.exit(main())

"""Bit-for-bit comparison of two builds of the library over everything the derived-state tables feed.

    python profiles/derived_tables_bitwise.py --parent PARENT.so [--new NEW.so] [--also NAME=OTHER.so] [--out FILE.json]

Each build runs in a fresh process of its own (the library is loaded once per process, through SIGGAN_LIB_PATH).  For every
seeded configuration below: three train_steps (clipping on the second, the next real batch staged, z and dropout from the
library RNG), then an eval g_forward, a d_forward, one g_latent_objective_grad and one g_compute_grads.  Recorded: the sha256
of every arena (params, grads, both moments, step counts), the BatchNorm running statistics and counters, the spectral-norm
u / v, every step's metrics buffer and the four outputs.  A call a context refuses (the latent objective on a 16-bit one) is
recorded by its message, which must be equal too.  --also: further builds held to the same hashes; what they print to
stderr behind the prefix TABLECMP is kept in the result (a scratch build that compares its job tables with the parent's
builders reports there)."""
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


def child(out_path):
    import torch
    sys.path.insert(0, ROOT)
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd.engine import Engine

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    res = {}
    for name, kw, B, extra in CONFIGS:
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
            clip = 1.0 if i == 1 else None
            if extra.get("ablation"):
                eng.d_compute_grads(reals[i], mask_passes=3)
                eng.d_apply(clip=clip)
                eng.g_compute_grads(B)
                eng.g_apply(clip=clip)
            else:
                eng.train_step(reals[i], clip=clip, next_real=reals[i + 1])
            torch.cuda.synchronize()
            r[f"step{i}/metrics"] = sha(eng.metrics)
        calls = {
            "g_forward": lambda: eng.g_forward(z, training=False),
            "d_forward": lambda: eng.d_forward(reals[3], training=False),
            "g_latent_objective_grad": lambda: torch.cat([t.reshape(-1) for t in eng.g_latent_objective_grad(
                z, target=reals[3], recon_weight=1.0, realism_weight=0.5, prior_weight=0.25, want_terms=True, want_probs=True)]),
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
    with open(out_path, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new", default=os.path.join(ROOT, "signature-gan_amd", "libsiggan_hip.so"))
    ap.add_argument("--also", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived_tables_bitwise.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    builds = [("parent", a.parent), ("new", a.new)] + [tuple(s.split("=", 1)) for s in a.also]
    got, notes = {}, {}
    for name, path in builds:
        tmp = a.out + "." + name + ".tmp"
        env = dict(os.environ, SIGGAN_LIB_PATH=os.path.abspath(path))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=env, capture_output=True, text=True, timeout=540)
        if p.returncode != 0:
            print(name, "FAILED", p.returncode, p.stderr[-2000:], flush=True)
            return 1
        got[name] = json.load(open(tmp))
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
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ("builds", "values_per_build", "all_equal", "different", "stderr_notes")}), flush=True)
    return 0 if not different else 1


if __name__ == "__main__":
    sys.exit(main())

"""Differential sweep of the training scope: every training sizer (and the dropout search's) of this build against another build's
``libovc.so`` over randomly mutated model descriptors and shapes.  A sizer answers 0 for what its entry point refuses and the
workspace bytes otherwise, so equal answers mean the same scope and the same layout size.  Host code only: no GPU is touched.

    python -m tools.train_scope_diff --against /path/to/other/libovc.so [--cases 4000] [--seed 20261021] [--out profiles/x.json]

Each case aims at one architecture (a valid descriptor of it), then mutates it: the encoder / decoder kinds, ``memory``,
``n_levels``, ``precision``, the per-site gates and memory slots (half pairs included), ``d_g`` / ``trig`` / the encoder's heads,
the meshed decoder's ``alpha`` gates, the vocabulary on either side of the fused tail's limit, ``d_model``, ``d_ff``; and draws a
shape, now and then one at a descriptor limit.  Prints one JSON line: the cases, the differences (the first few spelled out), and
per sizer how many of the cases aimed at its architecture it accepted -- the sweep fails (exit 1) on any difference, and when a
sizer accepts less than a tenth of them (the draw would be vacuous)."""
import argparse
import ctypes
import json
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from openviic_amd import native, train_arch  # noqa: E402

FAKE = 4096
AIMS = ("plain", "camo", "memory", "meshed", "geometric", "aoa")

# cell -> (sizer, its arguments behind the model from (B, N, T, S), the aims whose models it is meant to accept)
CELLS = {
    "train": ("ovc_train_workspace_bytes", lambda B, N, T, S: (B, N, T), ("plain", "camo", "memory")),
    "dropout": ("ovc_train_dropout_workspace_bytes", lambda B, N, T, S: (B, N, T), ("plain", "memory")),
    "beams": ("ovc_train_beams_workspace_bytes", lambda B, N, T, S: (B, N, S, T), ("plain", "camo", "memory")),
    "beams_dropout": ("ovc_train_beams_dropout_workspace_bytes", lambda B, N, T, S: (B, N, S, T), ("plain", "memory")),
    "search_dropout": ("ovc_beam_search_dropout_workspace_bytes", lambda B, N, T, S: (B, N, S), ("plain", "memory")),
}
for _flag in (0, 1):
    for _name in ("smoothed", "distill"):
        CELLS["%s/%d" % (_name, _flag)] = ("ovc_train_%s_workspace_bytes" % _name, lambda B, N, T, S, f=_flag: (B, N, T, f),
                                           ("plain", "memory") if _flag else ("plain", "camo", "memory"))
for _arch in train_arch.TRAIN_ARCHS.values():
    for _flag in (0, 1) if _arch.loss_dropout else (None,):
        CELLS[_arch.key if _flag is None else "%s/%d" % (_arch.key, _flag)] = (
            _arch.loss_form[0], lambda B, N, T, S, f=_flag: (B, N, T) if f is None else (B, N, T, f), (_arch.key,))
    CELLS[_arch.key + "_beams"] = (_arch.sequence_form[0], lambda B, N, T, S: (B, N, S, T), (_arch.key,))


def load(path):
    lib = ctypes.CDLL(path)
    for sizer, _, _ in CELLS.values():
        fn = getattr(lib, sizer)
        fn.restype, fn.argtypes = native.SIGNATURES[sizer]
    return lib


def base(aim):
    """A descriptor the aim's sizers accept: the yaml geometry (d = 512, 8 x 64 heads, three layers, V = 10201, 20 positions),
    fake pointers (a sizer dereferences none)."""
    d = native.Model()
    d.abi = native.ABI_VERSION
    d.enc_kind, d.dec_kind = native.ENC_PLAIN, native.DEC_PLAIN
    d.d_feat, d.d_model, d.heads, d.d_k, d.d_v, d.d_ff = 2048, 512, 8, 64, 64, 2048
    d.enc_heads, d.enc_d_k, d.enc_d_v = 8, 64, 64
    d.n_enc = d.n_dec = 3
    d.n_levels, d.memory, d.vocab, d.max_len = 1, 0, 10201, 20
    d.pad_idx, d.bos_idx, d.eos_idx, d.ln_eps = 0, 1, 2, 1e-5

    def lin(l):
        l.w = l.b = FAKE
    lin(d.proj)
    for i in range(native.OVC_MAX_LAYERS):
        for mha in (d.enc[i].att, d.dec[i].self_att, d.dec[i].cross_att):
            for name in "qkvo":
                lin(getattr(mha, name))
        for ffn in (d.enc[i].ffn, d.dec[i].ffn):
            lin(ffn.fc1); lin(ffn.fc2)
    if aim == "camo":
        d.enc_kind, d.enc_heads = native.ENC_CROSS_LEVEL, 1
        for name in "qkvo":
            lin(getattr(d.cl_att, name))
        lin(d.cl_mlp1); lin(d.cl_mlp2)
    if aim in ("memory", "meshed"):
        d.memory = 40
        for i in range(native.OVC_MAX_LAYERS):
            d.enc[i].att.m_k = d.enc[i].att.m_v = FAKE
    if aim == "meshed":
        d.enc_kind, d.dec_kind, d.n_levels = native.ENC_MULTILEVEL, native.DEC_MESHED, 3
        for i in range(native.OVC_MAX_LAYERS):
            for lvl in range(3):
                lin(d.dec[i].alpha[lvl])
    if aim == "geometric":
        d.enc_kind, d.d_g, d.trig, d.fc_g_w, d.fc_g_b = native.ENC_GEOMETRIC, 64, 1, FAKE, FAKE
    if aim == "aoa":
        for i in range(native.OVC_MAX_LAYERS):
            for mha in (d.enc[i].att, d.dec[i].self_att, d.dec[i].cross_att):
                lin(mha.aoa_i); lin(mha.aoa_g)
    return d


def mutate(d, aim, rng, rate):
    """Every mutation with probability ``rate`` (a few of them with a multiple of it, where most outcomes stay in scope)."""
    hit = lambda scale=1.0: rng.random() < rate * scale
    sites = [m for i in range(3) for m in (d.enc[i].att, d.dec[i].self_att, d.dec[i].cross_att)]
    if hit():
        d.enc_kind = rng.choice((native.ENC_PLAIN, native.ENC_MULTILEVEL, native.ENC_GEOMETRIC, native.ENC_CROSS_LEVEL))
    if hit():
        d.dec_kind = rng.choice((native.DEC_PLAIN, native.DEC_MESHED))
    if hit():
        d.memory = rng.choice((0, 1, 40))
    if hit():
        d.n_levels = rng.choice((1, 2, 3, 4))
    if hit(0.5):
        d.n_enc = rng.choice((1, 2, 3, 4))
    if hit(0.5):
        d.precision = rng.choice((3, 4))
    if hit(3) and aim == "meshed":       # the scope takes the multilevel encoder with and without slots
        d.memory = 0
        for i in range(native.OVC_MAX_LAYERS):
            d.enc[i].att.m_k = d.enc[i].att.m_v = None
    if hit(4) and aim == "aoa":          # ... and any subset of gated sites
        keep = rng.choice(("enc", "self", "cross", "some"))
        for i in range(native.OVC_MAX_LAYERS):
            for where, mha in (("enc", d.enc[i].att), ("self", d.dec[i].self_att), ("cross", d.dec[i].cross_att)):
                if where != keep and not (keep == "some" and rng.random() < 0.5):
                    mha.aoa_i.w = mha.aoa_i.b = mha.aoa_g.w = mha.aoa_g.b = None
    for _ in range(3):
        if hit(0.5):                     # one site: a gate pair or half of it, memory slots or half of them, set or cleared
            mha, value = rng.choice(sites), rng.choice((None, FAKE))
            for field in rng.choice((("aoa_i", "aoa_g"), ("aoa_i",), ("aoa_g",), ("m_k", "m_v"), ("m_k",), ("m_v",))):
                if field.startswith("aoa"):
                    getattr(mha, field).w = value
                else:
                    setattr(mha, field, value)
    if hit(2) and aim == "geometric":
        d.trig = rng.choice((0, 1))
        d.d_g = rng.choice((4, 4, 8, 16, 64, 64, 12, 72, 0)) if hit(20) else (64 if d.trig else 4)
    if hit():
        d.enc_heads = rng.choice((1, 4, 8, 16, 32))
        d.enc_d_k = d.enc_d_v = 64 if d.enc_heads <= 16 else 32
    if hit():
        d.fc_g_w, d.fc_g_b = rng.choice(((None, FAKE), (FAKE, None), (None, None), (FAKE, FAKE)))
    if hit():
        d.dec[rng.randrange(3)].alpha[rng.randrange(native.OVC_MAX_LEVELS)].w = rng.choice((None, FAKE))
    if hit(2):
        d.vocab = rng.choice((16384, 16385, 16383, 53, 2, 20000))
    if hit(2):
        d.d_model = rng.choice((64, 256, 1024, 2048, 2052, 48, 520))
    if hit():
        d.d_ff = rng.choice((128, 4096, 1 << 16, 1 << 20))
    if hit(0.5):
        d.cl_att.aoa_i.w = d.cl_att.aoa_g.w = rng.choice((None, FAKE))
    return d


LIMIT_SHAPES = [(51312, 1, 1, 1), (51313, 1, 1, 1), (52333, 1, 1, 1), (43626, 2, 1, 1), (43627, 2, 1, 1), (255, 1024, 1, 1),
                (256, 1024, 1, 1), (2565, 3, 20, 1), (2566, 3, 20, 1), (87253, 1, 1, 1), (4, 1024, 20, 5), (4, 1025, 20, 5),
                (4, 50, 21, 5), (0, 50, 20, 5), (4, 50, 0, 5), (4, 50, 20, 0), (4, 50, 20, 9), (1 << 24, 1, 1, 2)]


def draw_shape(rng):
    if rng.random() < 0.15:
        return rng.choice(LIMIT_SHAPES)
    return rng.choice((1, 3, 4, 60, 256)), rng.choice((1, 7, 50, 129, 1024)), rng.randint(1, 20), rng.randint(1, 8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--against", required=True, help="the other build's libovc.so")
    ap.add_argument("--cases", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--rate", type=float, default=0.04, help="the base probability of each mutation")
    ap.add_argument("--out", default="", help="merge the result into this JSON file under 'scope_diff'")
    args = ap.parse_args()
    mine, other = load(native.LIBRARY_PATH), load(args.against)
    rng = random.Random(args.seed)
    aimed = {cell: 0 for cell in CELLS}
    accepted = {cell: 0 for cell in CELLS}
    differences = []
    for case in range(args.cases):
        aim = AIMS[case % len(AIMS)]
        d = mutate(base(aim), aim, rng, args.rate)
        shape = draw_shape(rng)
        for cell, (sizer, arguments, aims) in CELLS.items():
            a = getattr(mine, sizer)(ctypes.byref(d), *arguments(*shape))
            b = getattr(other, sizer)(ctypes.byref(d), *arguments(*shape))
            if a != b:
                differences.append(dict(case=case, aim=aim, shape=shape, cell=cell, this=a, other=b))
            if aim in aims:
                aimed[cell] += 1
                accepted[cell] += a != 0
    vacuous = [cell for cell in CELLS if accepted[cell] * 10 < aimed[cell]]
    result = dict(cases=args.cases, seed=args.seed, rate=args.rate, cells=len(CELLS), sizers=len({s for s, _, _ in CELLS.values()}),
                  differences=len(differences), first_differences=differences[:8],
                  accepted={cell: "{}/{}".format(accepted[cell], aimed[cell]) for cell in CELLS}, vacuous=vacuous)
    print(json.dumps(result))
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                merged = json.load(f)
        merged["scope_diff"] = result
        with open(args.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
    return 1 if differences or vacuous else 0


if __name__ == "__main__":
    sys.exit(main())

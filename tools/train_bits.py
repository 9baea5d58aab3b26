"""The bits of every training call, as SHA-256 digests: every trainable architecture through every form its backward has, at the
tests' tiny configurations (B = 3, ragged N <= 9, T = 6, S = 2).  Two builds that run the same launch sequences write the same
file, so a refactor of the training path is checked by running this once per build on one machine and comparing the files.

    python -m tools.train_bits --out profiles/train_bits_<build>.json

Forms: ``xe`` (the NLL), ``xe_dropout`` (fixed seed), ``smoothed``, ``distill``, ``sequence`` (row weights on given ids) and
``sequence_dropout`` (the ids, slots and masks of a dropout search with the same seed) -- each where the architecture has it.
Every form runs three calls with ``use_graph`` on (the third replays the captured body) and one with it off; each call's loss
(or recomputed log-probabilities) and every gradient tensor is hashed.  A call's row holds the digest of its head and ONE digest
over its gradients -- the SHA-256 of the tensors' own digests, concatenated in ``gradient_parameters()`` order; ``--tensors``
lists the per-tensor digests as well, to find which tensor two builds differ in.  Uses only the engine's public methods."""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from openviic_amd import dropout as D  # noqa: E402
from openviic_amd.builders import build_model  # noqa: E402
from openviic_amd.config import model_config  # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_boxes, synthetic_features, synthetic_state_dict  # noqa: E402

TINY = dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=2, memory=5)
B, V, T, S = 3, 53, 6, 2
PAD, BOS, EOS = 0, 1, 2
# variant -> (the keyword of its training calls, model_config overrides, N, the forms it has)
PLAIN_FORMS = ("xe", "xe_dropout", "smoothed", "distill", "sequence", "sequence_dropout")
VARIANTS = {
    "standard_transformer": ({}, {}, 7, PLAIN_FORMS),
    "augmented_memory_transformer": ({}, {}, 7, PLAIN_FORMS),
    "camo_transformer": ({}, dict(enc_heads=4, layers=3), 9, ("xe", "smoothed", "distill", "sequence")),
    "meshed_memory_transformer": (dict(meshed=True), {}, 7, ("xe", "sequence")),
    "object_relation_transformer": (dict(geometric=True), {}, 7, ("xe", "xe_dropout", "sequence")),
    "attention_on_attention": (dict(aoa=True), {}, 7, ("xe", "xe_dropout", "sequence")),
}


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def build(variant, dims, N):
    dims = dict(TINY, **dims)
    vocab = SyntheticVocab(V, T)
    cfg = model_config(variant, device="cuda:0", **dims)
    model = build_model(cfg, vocab)
    sd = synthetic_state_dict(model.state_dict(), seed=11, mode="generic", memory_dims=(dims["d_kv"], dims["memory"]))
    model.load_state_dict(sd, strict=False)
    feats = synthetic_features(B, N, dims["d_feature"], seed=3, ragged=True).cuda()
    boxes = synthetic_boxes(B, N, seed=3).cuda() if variant == "object_relation_transformer" else None
    return model, feats, boxes


def tokens():
    g = torch.Generator().manual_seed(88)
    tok = torch.randint(4, V, (B, T), generator=g)
    tok[:, 0] = BOS
    tok[0, T - 2:] = PAD
    tok[1, 2] = PAD
    targets = torch.cat([tok[:, 1:], torch.full((B, 1), PAD, dtype=tok.dtype)], 1)
    return tok.cuda(), targets.cuda()


def sequences():
    g = torch.Generator().manual_seed(89)
    ids = torch.randint(4, V, (B, S, T), generator=g)
    ids[0, 0, 3] = EOS          # ragged ends: rows behind a first <eos> carry no gradient
    ids[1, 1, T - 1] = EOS
    ids[2, 0, 1] = EOS
    return ids.cuda(), torch.randn(B, S, T, generator=g).cuda()


def run_form(call, tensors):
    """Three calls on the graph path (issue, capture, replay), then one with plain launches: the digests of each."""
    out = {}
    for name, graph in (("graph_1", True), ("graph_2", True), ("graph_3", True), ("plain", False)):
        head, grads = call(graph)
        torch.cuda.synchronize()
        each = [digest(g) for g in grads]
        out[name] = dict(head=digest(head), grads=hashlib.sha256("".join(each).encode()).hexdigest())
        if tensors:
            out[name]["tensors"] = each
    return out


def dump(value, depth=0):
    """JSON with sorted keys, one call's digests per line."""
    if not isinstance(value, dict) or all(isinstance(v, (str, list)) for v in value.values()):
        return json.dumps(value, sort_keys=True)
    pad = " " * (depth + 1)
    return "{\n" + ",\n".join("{}{}: {}".format(pad, json.dumps(k), dump(v, depth + 1)) for k, v in sorted(value.items())) + "\n" + pad[1:] + "}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--tensors", action="store_true", help="also list every gradient tensor's own digest")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    tok, targets = tokens()
    ids, weights = sequences()
    seed = torch.tensor([20261021], dtype=torch.int64, device="cuda:0")
    g = torch.Generator().manual_seed(90)
    teacher = torch.log_softmax(torch.randn(B, T, V, generator=g), -1).cuda().contiguous()
    result = {}
    for variant, (kw, dims, N, forms) in VARIANTS.items():
        model, feats, boxes = build(variant, dims, N)
        model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.1
        eng = model._fused_engine()
        probs = D.model_probs(model) if any("dropout" in f for f in forms) else None

        def loss_call(**more):
            def call(graph):
                loss, _, grads = eng.forward_backward(feats, boxes, tok, targets, use_graph=graph, **kw, **more)
                return loss, grads
            return call

        def sequence_call(ids_, **more):
            def call(graph):
                _, grads, logp = eng.sequence_backward(feats, boxes, ids_, weights, use_graph=graph, want_logp=True, **kw, **more)
                return logp, grads
            return call
        rows = {}
        for form in forms:
            if form == "xe":
                rows[form] = run_form(loss_call(), args.tensors)
            elif form == "xe_dropout":
                rows[form] = run_form(loss_call(dropout=(probs, seed)), args.tensors)
            elif form == "smoothed":
                rows[form] = run_form(loss_call(loss=(0.1, "mean")), args.tensors)
            elif form == "distill":
                rows[form] = run_form(loss_call(distill=(teacher, 0.5)), args.tensors)
            elif form == "sequence":
                rows[form] = run_form(sequence_call(ids), args.tensors)
            elif form == "sequence_dropout":
                found, _, slots = eng.beam_search(feats, boxes, B, S, out_size=S, dropout=(probs, seed))
                rows[form] = dict(search=digest(found),       # not the slots: behind a beam's first <eos> they are unspecified
                                  **run_form(sequence_call(found, dropout=(probs, seed), slots=slots, beam_size=S), args.tensors))
        result[variant] = dict(gradients=len(eng.gradient_parameters()), forms=rows)
        print(variant, {form: rows[form]["plain"]["head"][:12] for form in rows}, flush=True)
    with open(args.out, "w") as f:
        f.write(dump(result) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

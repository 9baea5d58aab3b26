#!/usr/bin/env python3
"""Full graph vs early_exit=True (host-driven, blocking) vs early_exit="device" (gated launches in one graph), same process, modes
alternated.  Full-size standard model (d2048 features, 50 regions, beam 5, V = 10201) with EOS-biased weights unless noted.

    python tools/device_early_exit_probe.py [out.json] [reps=20]

Rows: (a) one resident stream at B = 1 / 8 / 32 / 256; (b) the prediction loop over feature files at B = 1 and 8, 4 slots;
(c) B = 256 on 4 streams; (d) max_len 128 and 256 at B = 1 and 256; (e) weights that never emit <eos> (the bench workload),
gated vs ungated graph.  Prints one JSON object per row and writes them all to out.json.
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.instance import InstanceList
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict

MODES = (False, True, "device")


def make_model(T=20, eos=True):
    vocab = SyntheticVocab(10201, T)
    model = build_model(model_config("standard_transformer", d_feature=2048, device="cuda:0"), vocab).eval()
    sd = synthetic_state_dict(model.state_dict(), seed=1234, mode="reference_init")
    if eos:
        sd = eos_biased_state_dict(sd, model.state_dict(), mid=min(10, T // 2))
    model.load_state_dict(sd, strict=False)
    return model, vocab


def items_of(B, seed=0):
    it = InstanceList()
    it.region_features = synthetic_features(B, 50, 2048, seed=seed).cuda()
    return it


def resident(model, B, mode, reps, streams=1):
    batches = [items_of(B, seed=s) for s in range(streams)]
    ss = [torch.cuda.Stream() for _ in range(streams)]
    with torch.no_grad():
        for _ in range(3):
            for it, s in zip(batches, ss):
                with torch.cuda.stream(s):
                    model.beam_search(it, batch_size=B, beam_size=5, early_exit=mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            for it, s in zip(batches, ss):
                with torch.cuda.stream(s):
                    model.beam_search(it, batch_size=B, beam_size=5, early_exit=mode)
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng = model._engine
    steps = int(eng.last_steps_device.item()) if mode == "device" else eng.last_steps_run
    return {"ms_per_batch": 1e3 * dt / (reps * streams), "captions_per_s": reps * streams * B / dt, "steps": steps}


def loop(model, vocab, B, mode, paths):
    from openviic_amd.data import predict_feature_files
    predict_feature_files(model, vocab, paths[:8], batch_size=B, beam_size=5, slots=4, early_exit=mode)     # warm shapes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = predict_feature_files(model, vocab, paths, batch_size=B, beam_size=5, slots=4, early_exit=mode)
    torch.cuda.synchronize()
    return {"captions_per_s": len(out) / (time.perf_counter() - t0)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "device_early_exit.json"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    model, _ = make_model()
    for B in (1, 8, 32, 256):
        for mode in MODES:
            emit(dict(row="a", B=B, mode=mode, **resident(model, B, mode, reps if B < 256 else max(4, reps // 4))))
    for mode in MODES:
        emit(dict(row="c", B=256, streams=4, mode=mode, **resident(model, 256, mode, max(3, reps // 6), streams=4)))
    from openviic_amd.vocab import WordVocab
    words = WordVocab(["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(4, 10201)], 20)
    with tempfile.TemporaryDirectory() as tmp:
        g = np.random.default_rng(3)
        paths = []
        for i in range(192):
            p = os.path.join(tmp, "img_%03d.npz" % i)
            np.savez(p, region_features=g.standard_normal((50, 2048), dtype=np.float32))
            paths.append(p)
        for B in (1, 8):
            for mode in MODES:
                emit(dict(row="b", B=B, slots=4, mode=mode, **loop(model, words, B, mode, paths)))
    del model
    for T in (128, 256):
        model, _ = make_model(T=T)
        for B in (1, 256):
            for mode in MODES:
                emit(dict(row="d", max_len=T, B=B, mode=mode, **resident(model, B, mode, max(3, reps // (4 if B == 1 else 10)))))
        del model
    model, _ = make_model(eos=False)
    for B in (1, 256):
        for _ in range(2):
            for mode in (False, "device"):
                emit(dict(row="e", B=B, mode=mode, never_eos=True, **resident(model, B, mode, reps if B == 1 else max(4, reps // 4))))
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

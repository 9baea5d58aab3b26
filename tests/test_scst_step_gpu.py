"""The self-critical iteration in one call (``model.scst_step``) and its one new kernel (``ovc_scst_advantage``,
``openviic_amd.scst.advantage``).

Kernel: ``grad_logp`` bit for bit against the numpy mirror, ``stats`` within ``2^-23 |x| + 1e-12 sum |terms|`` of the mirror's
float64 values; the same bits on every call, stream and graph replay.  Step: parameters and Adam state bit for bit against the
reference's lines on a second copy of the model; the step arena's gradients on the bar of ``test_scst_gpu._check`` against the
float64 oracle and the reference's recorded gradients; the same bits for every search form and with graph replay on and off;
every refusal before any launch and any random draw."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import TINY_SHAPE, batch, device_model, golden, tiny_case
from openviic_amd import native, scst
from openviic_amd.builders import build_model
from openviic_amd.cider import CiderCorpus
from openviic_amd.config import model_config
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
from openviic_amd.vocab import WordVocab
from scst_oracle import scst_gradients
from test_scst_gpu import _check, _eos_sd, _named
from test_scst_step_cpu import SHAPES, inputs, stats_bound

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMO_TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
K = TINY_SHAPE["k"]
ROWS = [34, 23, 38]         # corpus images whose references share words with the tiny model's captions: the rewards differ


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# -- 1. the kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_advantage_matches_the_mirror(shape):
    B, S, T = shape
    reward, logp = inputs(B, S, T)
    want_g, _, want64 = scst.mirror_advantage(reward, logp)
    r, x = torch.from_numpy(reward).cuda(), torch.from_numpy(logp).cuda()
    grad, stats = scst.advantage(r, x)
    assert grad.dtype == torch.float32 and tuple(grad.shape) == shape and tuple(stats.shape) == (4,)
    assert np.array_equal(grad.cpu().numpy().view(np.int32), want_g.view(np.int32))
    got = stats.cpu().numpy().astype(np.float64)
    r64 = reward.astype(np.float64)
    term = -(logp.astype(np.float64).mean(-1)) * (r64 - r64.mean(-1, keepdims=True)) / (B * S)
    for q, terms in ((0, term), (1, r64 / (B * S)), (2, r64 / (B * S))):
        print("%s stats[%d]: device %.9g, float64 mirror %.17g" % (shape, q, got[q], want64[q]))
        assert abs(got[q] - want64[q]) <= stats_bound(want64[q], terms), (shape, q, got[q], want64[q])
    assert got[3] == 0
    # the same bits on a second call, on a second stream, and captured in a graph and replayed
    again = scst.advantage(r, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = scst.advantage(r, x)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = scst.advantage(r, x)
    for _ in range(2):
        captured[0].zero_()
        captured[1].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for pair in (again, other, captured):
            assert _bits(pair[0], grad) and _bits(pair[1], stats)


def test_advantage_exact_zeros_and_host_refusals():
    reward, logp = inputs(5, 4, 9)
    reward[1] = 7.3
    reward[3] = 0.0
    grad, _ = scst.advantage(torch.from_numpy(reward).cuda(), torch.from_numpy(logp).cuda())
    assert not bool(grad[1].any()) and not bool(grad[3].any()) and bool(grad[0].any())
    reward, logp = inputs(6, 1, 11)
    grad, stats = scst.advantage(torch.from_numpy(reward).cuda(), torch.from_numpy(logp).cuda())
    assert not bool(grad.any()) and float(stats[0]) == 0
    r, x = torch.from_numpy(reward).cuda(), torch.from_numpy(logp).cuda()
    for bad_r, bad_x in ((r.double(), x), (r, x.transpose(1, 2)), (r[:, :0], x[:, :0]), (r.cpu(), x)):
        with pytest.raises(native.OvcError):
            scst.advantage(bad_r, bad_x)
    with pytest.raises(native.OvcError, match="contiguous"):
        scst.advantage(torch.zeros(4, 6, device="cuda")[:, ::2], torch.zeros(4, 3, 5, device="cuda"))


# -- 2. the step -------------------------------------------------------------------------------------------------------------
def _no_dropout(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def _case(variant):
    """(config, vocab, EOS-biased state dict, features) of a tiny case of ``variant``."""
    if variant == "camo_transformer":
        vocab = SyntheticVocab(53, 6)
        cfg = model_config("camo_transformer", device="cpu", **CAMO_TINY)
        sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
        feats = synthetic_features(3, 9, CAMO_TINY["d_feature"], seed=3, ragged=True)
    else:
        cfg, vocab, sd, feats, _ = tiny_case(variant)
    return cfg, vocab, _eos_sd(cfg, vocab, sd, mid=3), feats


def _corpus():
    with open(os.path.join(REPO, "tests", "golden", "g18_cider_reward.json")) as f:
        g = json.load(f)
    return CiderCorpus(WordVocab(g["words"], 20), g["df_corpus"], g["references"]).to("cuda")


def _seeded_reward(outs):
    """A reward that is a fixed function of the ids, in [0, 10): both forms of the step see the same values."""
    weights = torch.arange(1, outs.shape[-1] + 1, device=outs.device)
    return ((outs * weights).sum(-1) % 97).float() / 9.7


def _lines(model, optimizer, items, B, k, reward, dropout=False, early_exit=None):
    """The iteration ``scst_step`` stands for."""
    outs, log_probs = model.beam_search(items, B, k, out_size=k, dropout=dropout, early_exit=early_exit)
    optimizer.zero_grad()
    r = reward(outs)
    g, stats = scst.advantage(r, log_probs.detach())
    log_probs.backward(g)
    optimizer.step()
    return outs, r, stats


def _state_bits_equal(model_a, opt_a, model_b, opt_b):
    for (name, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert _bits(pa.detach(), pb.detach()), name
        sa, sb = opt_a.state.get(pa, {}), opt_b.state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (_bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)


@pytest.mark.parametrize("variant,dropout,reward", [("standard_transformer", False, "corpus"), ("standard_transformer", True, "corpus"),
                                                    ("augmented_memory_transformer", False, "seeded"),
                                                    ("camo_transformer", False, "seeded")])
def test_scst_step_leaves_the_bits_of_the_lines(variant, dropout, reward):
    cfg, vocab, sd, feats = _case(variant)
    B = feats.shape[0]
    models = [device_model(cfg, vocab, sd) for _ in range(2)]
    for m in models:
        if dropout:
            m.train()
            for mod in m.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.1
        else:
            _no_dropout(m)
        m.decoder.layers[0].pwff.fc1.bias.requires_grad_(False)          # a frozen parameter is not updated by either form
    opts = [Adam(_trainable(m), lr=1e-3, betas=(0.9, 0.98)) for m in models]
    items = batch(feats)
    if reward == "corpus":                   # the tiny vocabulary (53 ids) lies inside the corpus' (60 words)
        corpus = _corpus()
        rows = torch.tensor(ROWS, dtype=torch.int32, device="cuda")
        by_lines, in_step = (lambda outs: corpus.reward(outs, rows)), corpus
    else:
        rows, by_lines, in_step = None, _seeded_reward, _seeded_reward
    for i in range(3):
        torch.manual_seed(40 + i)
        outs, r, stats = _lines(models[0], opts[0], items, B, K, by_lines, dropout=dropout)
        torch.manual_seed(40 + i)
        with torch.no_grad() if i == 1 else torch.enable_grad():
            out = models[1].scst_step(items, opts[1], in_step, K, rows=rows, dropout=dropout)
        assert torch.equal(out.outs, outs) and _bits(out.reward, r)
        for got, want in zip(out[:3], stats[:3]):
            assert got.dim() == 0 and not got.requires_grad and _bits(got, want)
        assert bool(r.std() > 0), "the rewards must differ inside an image"
    assert all(p.grad is None for p in models[1].parameters())
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    assert not _bits(models[1].decoder.fc.weight.detach(), sd["decoder.fc.weight"].cuda())
    assert all(float(opts[1].state[p]["step"]) == 3 for p in _trainable(models[1]))


@pytest.mark.parametrize("case", ["g1", "eos"])
def test_step_arena_gradients_match_reference_and_fp64_oracle(case):
    g = golden("g16_tiny_standard_transformer_scst_%s.npz" % case)
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    if case == "eos":
        sd = _eos_sd(cfg, vocab, sd, mid=3)
    model = _no_dropout(device_model(cfg, vocab, sd))
    B = feats.shape[0]
    reward = torch.from_numpy(g["reward"])
    before = [p.detach().clone() for p in model.parameters()]
    out = model.scst_step(batch(feats), Adam(_trainable(model), lr=0.0), lambda outs: reward.cuda(), K)
    assert all(_bits(a, p.detach()) for a, p in zip(before, model.parameters())), "lr = 0 leaves the parameters as they are"
    assert torch.equal(out.outs.cpu(), torch.from_numpy(g["ids"]))
    adv = (reward - reward.mean(-1, keepdim=True)).abs().mean()
    print("G16 %s: loss %.9g, recorded %.9g" % (case, out.loss.item(), float(g["loss"])))
    assert abs(out.loss.item() - float(g["loss"])) <= 1e-5 * float(adv) + 1e-7
    eng = model._fused_engine()
    got = {n: v for n, v in _named(eng, eng.step_arena()[2]).items() if dict(model.named_parameters())[n].requires_grad}
    ref = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    _, _, g64 = scst_gradients(cfg, sd, vocab, feats, out.outs.cpu(), reward)
    _, _, g32 = scst_gradients(cfg, sd, vocab, feats, out.outs.cpu(), reward, dtype=torch.float32)
    eps, worst = _check(got, g64, g32, extra=ref)
    print("G16 %s through scst_step: eps %.2e, worst gap to fp64 oracle / reference %.2e" % (case, eps, worst))


def test_search_forms_and_graph_replay_give_the_same_bits():
    cfg, vocab, sd, feats = _case("standard_transformer")
    B = feats.shape[0]
    items = batch(feats)
    results = []
    for early_exit, use_graph in ((False, True), (True, True), ("device", True), (False, False)):
        model = _no_dropout(device_model(cfg, vocab, sd))
        model._fused_engine().use_graph = use_graph
        opt = Adam(_trainable(model), lr=1e-3)
        for _ in range(3):                           # first call plain, second captured, third replayed
            out = model.scst_step(items, opt, _seeded_reward, K, early_exit=early_exit)
        results.append((model, opt, out))
    for model, opt, out in results[1:]:
        _state_bits_equal(results[0][0], results[0][1], model, opt)
        assert torch.equal(out.outs, results[0][2].outs) and _bits(out.loss, results[0][2].loss)


def test_refusals_launch_nothing_and_draw_nothing():
    cfg, vocab, sd, feats = _case("standard_transformer")
    B = feats.shape[0]
    items = batch(feats)
    corpus = _corpus()

    def refused(model, match, make_optimizer=None, reward=_seeded_reward, **kw):
        before = [p.detach().clone() for p in model.parameters()]
        opt = (make_optimizer or (lambda: Adam(_trainable(model))))()
        rng = torch.cuda.get_rng_state()
        with pytest.raises(native.OvcError, match=match):
            model.scst_step(kw.pop("items", items), opt, reward, K, **kw)
        assert torch.equal(rng, torch.cuda.get_rng_state())
        assert all(p.grad is None for p in model.parameters())
        assert all(_bits(a, p.detach()) for a, p in zip(before, model.parameters()))
        assert not opt.state

    c, v, s, f, _ = tiny_case("meshed_memory_transformer")
    meshed = _no_dropout(device_model(c, v, s))
    refused(meshed, "plain", items=batch(f))
    refused(meshed.train(), "plain", items=batch(f), dropout=True)
    for m in meshed.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    refused(meshed, "plain", items=batch(f), dropout=True)
    live = device_model(cfg, vocab, sd).train()
    refused(live, "DROPOUT: 0")
    model = _no_dropout(device_model(cfg, vocab, sd))
    foreign = torch.nn.Parameter(torch.zeros(3, device="cuda"))
    refused(model, "exactly the model's trainable parameters", make_optimizer=lambda: Adam(_trainable(model) + [foreign]))
    refused(model, "openviic_amd.optim.Adam", make_optimizer=lambda: torch.optim.Adam(_trainable(model)))
    refused(model, "rows must be", reward=corpus, rows=torch.zeros(B, dtype=torch.int64, device="cuda"))
    refused(model, "rows must be", reward=corpus, rows=torch.zeros(B + 1, dtype=torch.int32, device="cuda"))
    refused(model, "rows must be", reward=corpus, rows=torch.zeros(B, dtype=torch.int32))
    on_host = CiderCorpus(WordVocab(["<pad>", "<bos>", "<eos>", "<unk>", "w0"], 20), {"0": ["w0"]}, [["w0"]])     # never moved
    refused(model, "move the corpus", reward=on_host, rows=torch.zeros(B, dtype=torch.int32, device="cuda"))
    refused(model, r"float32 \[3, 3\]", reward=lambda outs: torch.zeros(B, K - 1, device="cuda"))
    refused(model, r"float32 \[3, 3\]", reward=lambda outs: torch.zeros(B, K, device="cuda", dtype=torch.float64))
    refused(model, "CiderCorpus or a callable", reward=3.0)
    # the same model still steps
    opt = Adam(_trainable(model))
    out = model.scst_step(items, opt, corpus, K, rows=torch.zeros(B, dtype=torch.int32, device="cuda"))
    assert tuple(out.reward.shape) == (B, K) and all(float(opt.state[p]["step"]) == 1 for p in _trainable(model))

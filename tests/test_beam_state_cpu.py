"""The host restatement of the search's bookkeeping (``tests/beam_state_oracle.py``) and the case lists of
``tests/test_beam_state_gpu.py`` (``tests/beam_state_cases.py``), checked without a device.

* ``step_state`` chained over T steps and ``finalize("plain")`` / ``gather_all`` / ``masked_logp`` must reproduce a direct transcription
  of the reference's beam search (``models/modules/beam_search.py``: ``torch.sort(..., stable=True)`` and ``torch.gather``) exactly:
  ids, per-token log-probabilities and ``all_logp``;
* the forced, normalized, gated and plain orderings must equal a ``sorted(key=...)`` of the rule stated in ``include/ovc.h``;
* every precondition the GPU cases rely on holds: k finite candidates per image, no exact tie between winners of different rows, every
  generated index inside its table, the parents the cases are built to force, and the kernel list against the source text.
"""
import os
import re

import numpy as np
import pytest
import torch

import beam_state_cases as cases
import beam_state_oracle as oracle
from openviic_amd import prefix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EOS = cases.EOS


# ---- 1. the chain against the reference's search --------------------------------------------------------------------------------

def _tables(B, k, T, V, seed):
    """A toy model: the log-probabilities of step t depend on (t, image, beam slot).  <eos> is planted so that beams freeze."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, k, V, generator=g) * 2
    x[1:, :, 0, EOS] += 6                                   # slot 0 tends to end early, the others now and then
    x[2::2, :, k - 1, EOS] += 4
    return torch.log_softmax(x, -1)


def _reference_search(tables, k, out_size):
    """models/modules/beam_search.py:41-118, transcribed: the state is the step table's rows in slot order."""
    T, B, _, V = tables.shape
    seq_mask = torch.ones(B, k, 1)
    seq_logprob = torch.zeros(B, 1, 1)
    outputs, log_probs, all_log_probs = [], [], []
    selected_words = None
    for t in range(T):
        cur = 1 if t == 0 else k
        word_logprob = tables[t][:, :cur].clone()
        candidate = seq_logprob + word_logprob
        if t > 0:
            mask = (selected_words.view(B, cur) != EOS).float().unsqueeze(-1)
            seq_mask = seq_mask * mask
            word_logprob = word_logprob * seq_mask.expand_as(word_logprob)
            old = seq_logprob.expand_as(candidate).contiguous()
            old[:, :, 1:] = -999
            candidate = seq_mask * candidate + old * (1 - seq_mask)
        val, idx = torch.sort(candidate.view(B, -1), dim=-1, descending=True, stable=True)
        val, idx = val[:, :k], idx[:, :k]
        beam = torch.div(idx, V, rounding_mode="trunc")
        words = idx - beam * V
        seq_logprob = val.unsqueeze(-1)
        seq_mask = torch.gather(seq_mask, 1, beam.unsqueeze(-1))
        outputs = [torch.gather(o, 1, beam.unsqueeze(-1)) for o in outputs] + [words.unsqueeze(-1)]
        all_log_probs.append((word_logprob.expand(B, k, -1) if t == 0 else word_logprob).unsqueeze(2))
        this = torch.gather(torch.gather(word_logprob, 1, beam.unsqueeze(-1).expand(B, k, V)), 2, words.unsqueeze(-1))
        log_probs = [torch.gather(o, 1, beam.unsqueeze(-1).expand(B, k, 1)) for o in log_probs] + [this]
        selected_words = words.view(-1, 1)
    _, sort_idxs = torch.sort(seq_logprob, dim=1, descending=True, stable=True)
    ids = torch.gather(torch.cat(outputs, -1), 1, sort_idxs.expand(B, k, T))
    lp = torch.gather(torch.cat(log_probs, -1), 1, sort_idxs.expand(B, k, T))
    allp = torch.cat(all_log_probs, 2)
    allp = torch.gather(allp, 1, sort_idxs.unsqueeze(-1).expand(B, k, T, V))
    return ids[:, :out_size].numpy(), lp[:, :out_size].numpy(), allp.numpy()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("T,V,seed", [(7, 33, 1), (12, 53, 2)])
def test_chained_steps_and_plain_finalize_are_the_reference_search(k, T, V, seed):
    B = 3
    tables = _tables(B, k, T, V, seed)
    want_ids, want_lp, want_all = _reference_search(tables, k, k)
    running, alive = np.zeros(B, F32), np.ones(B, F32)
    hist, lp, anc = (np.zeros((B, T), dt) for dt in (np.int32, F32, np.int32))
    all_buf = np.zeros(T * B * k * V, F32)
    froze = False
    for t in range(T):
        W = 1 if t == 0 else k
        x = tables[t][:, :W].reshape(B * W, V).numpy()
        zero = np.zeros(B * W, F32)                          # the tables are log-probabilities already: (x - 0) - 0 is x
        row = oracle.masked_logp(x[None], zero[None], zero[None], alive)
        at = 0 if t == 0 else t * B * k * V
        all_buf[at:at + row.size] = row.reshape(-1)
        p, w, s = prefix.mirror_update(x, running, alive, k, t, None, np.zeros(B, np.int32), zero, zero)
        out = {"hist_out": np.full((B * k, T), -7, np.int32), "lp_out": np.full((B * k, T), 9, F32), "anc_out": np.full((B * k, T), -7, np.int32),
               "alive_out": np.full(B * k, 9, F32), "running_out": np.full(B * k, 9, F32), "next_tok": np.full(B * k, -7, np.int32)}
        st = oracle.step_state(out, x, alive, hist, lp, anc, p, w, s, zero, zero, k, t, EOS, cases.PAD)
        assert (st["hist_out"][:, t + 1:] == -7).all() and (st["lp_out"][:, t + 1:] == 9).all()      # nothing behind column t
        assert np.array_equal(st["next_tok"], st["hist_out"][:, t])
        running, alive, hist, lp, anc = st["running_out"], st["alive_out"], st["hist_out"], st["lp_out"], st["anc_out"]
        froze = froze or (alive == 0).any()
    assert froze or k == 1, "no beam ended: the case does not reach the frozen-beam path"
    for out_size in sorted({1, k}):
        fin = oracle.finalize("plain", running, hist, lp, k, out_size)
        assert np.array_equal(fin["ids"], want_ids[:, :out_size])
        assert np.array_equal(fin["logp"].view(np.int32), want_lp[:, :out_size].view(np.int32))      # bits: the frozen beams' signed zeros
    got_all = oracle.gather_all(all_buf, fin["order"], B, k, T, V)
    assert np.array_equal(got_all.view(np.int32), want_all.view(np.int32))


# ---- 2. the orderings against sorted(key=...) ------------------------------------------------------------------------------------

def _sorted_order(case, inp, b):
    k, T = case.k, case.T
    run = inp["running"][b * k:(b + 1) * k]
    if case.form == "forced":
        kb = k >> case.C
        return sorted(range(k), key=lambda j: (not run[j] > -np.inf, -bin(j // kb).count("1"), -run[j], j))
    if case.form == "normalized":
        L = np.clip(inp["len_in"][b * k:(b + 1) * k], 1, T)
        keys = ((run + inp["bonus"][L - 1]).astype(F32) * inp["inv"][L - 1]).astype(F32)
        return sorted(range(k), key=lambda j: (np.isnan(keys[j]), 0 if np.isnan(keys[j]) else -keys[j], 0 if np.isnan(keys[j]) else -run[j], j))
    return sorted(range(k), key=lambda j: (-run[j], j))


@pytest.mark.parametrize("case", cases.FINAL_CASES, ids=lambda c: "%s-k%d-o%d-T%d-%s" % (c.name, c.k, c.out_size, c.T, c.plant))
def test_orderings_are_the_stated_rule(case):
    B, k, T = 3, case.k, case.T
    inp = cases.final_inputs(case, B)
    state = (inp["running"], inp["hist"], inp["lp"])
    steps_run = case.steps_run
    fin = oracle.finalize(case.form, inp["running"], inp["hist"], inp["lp"], k, case.out_size, steps_run=case.steps_run,
                          other=(inp["running2"], inp["hist2"], inp["lp2"]), alive_count=inp["alive_count"], C=case.C, len_in=inp["len_in"],
                          inv=inp["inv"], bonus=inp["bonus"])
    if case.form == "gated":
        counts = inp["alive_count"]
        S = next((i + 1 for i in range(T - 1) if counts[i] == 0), T)
        assert S == {"first": 1 if T > 1 else T, "lanes": 71, "none": T}[case.counts]
        if S & 1:                                            # the state of buffer S & 1
            state = (inp["running2"], inp["hist2"], inp["lp2"])
            inp = dict(inp, running=inp["running2"])
        steps_run = S if S < T else 0
    if case.form != "normalized":
        assert not np.isnan(inp["running"]).any()            # the plain, gated and forced orderings are handed no NaN score
    written = steps_run if steps_run > 0 else T
    for b in range(B):
        want = _sorted_order(case, inp, b)
        assert fin["order"][b].tolist() == want
        for o in range(case.out_size):
            src = b * k + want[o]
            assert np.array_equal(fin["ids"][b, o, :written], state[1][src, :written]) and (fin["ids"][b, o, written:] == 0).all()
            assert np.array_equal(fin["logp"][b, o, :written], state[2][src, :written]) and (fin["logp"][b, o, written:] == 0).all()
    if case.form == "gated":
        assert fin["steps"] == S
    if case.plant == "neginf":
        assert fin["order"][0].tolist() == (list(range(k)) if case.form != "forced" else _sorted_order(case, inp, 0))
    if case.plant == "equal" and case.form in ("plain", "gated"):
        assert all(fin["order"][b].tolist() == list(range(k)) for b in range(B))
    if case.plant == "keys":
        assert fin["order"][0].tolist().index(1) + 1 == fin["order"][0].tolist().index(5)       # equal keys and scores: the lower slot
        run1 = inp["running"][k:2 * k]
        assert fin["order"][1].tolist() == sorted(range(k), key=lambda j: (-run1[j], j)) and len(set(fin["score"][1].tolist())) == 1
        assert fin["order"][2][-1] == 3 and np.isnan(fin["score"][2][-1])
        assert fin["len"][0][fin["order"][0].tolist().index(0)] == 3


def test_final_cases_cover_the_sizes_and_plants():
    for form in ("plain", "gated", "normalized"):
        got = {(c.k, c.out_size, c.T) for c in cases.FINAL_CASES if c.form == form}
        assert got >= set(cases.FINAL_SIZES)
        assert {c.plant for c in cases.FINAL_CASES if c.form == form} >= set(cases.PLANTS)
    assert {(c.k, c.C) for c in cases.FINAL_CASES if c.form == "forced"} == {(2, 1), (8, 2), (8, 3)}
    assert {c.plant for c in cases.FINAL_CASES if c.form == "forced"} == set(cases.PLANTS)
    plain = [c for c in cases.FINAL_CASES if c.form == "plain"]
    assert {0, 1} <= {c.steps_run for c in plain} and any(c.steps_run == c.T - 1 and c.T > 1 for c in plain)
    gated = [c for c in cases.FINAL_CASES if c.form == "gated"]
    assert {"first", "lanes", "none"} == {c.counts for c in gated} and any(c.T == 1 for c in gated)
    assert all(c.T == 130 for c in gated if c.counts == "lanes")
    assert {c.form for c in cases.FINAL_CASES} == set(cases.FINAL_FORMS)


# ---- 3. the step cases' preconditions ------------------------------------------------------------------------------------------

def test_kernel_list_is_the_source_text():
    """FOLLOW_KERNELS names exactly the kernels of beam.hip whose body -- its own text or the body file it includes -- calls
    beam_follow_winners, and the ids are the header's."""
    csrc = os.path.join(REPO, "openviic_amd", "csrc")
    text = open(os.path.join(csrc, "beam.hip")).read()
    found = set()
    for m in re.finditer(r"__global__[^;{]*?void\s+(\w+)\s*\(", text):
        start = text.index("{", text.index(")", m.end()))
        depth, i = 0, start
        while True:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            if depth == 0:
                break
            i += 1
        body = text[start:i]
        for inc in re.findall(r'#include "(bodies/\w+\.inc)"', body):
            body += open(os.path.join(csrc, inc)).read()
        if "beam_follow_winners<" in body:
            found.add(m.group(1))
    assert found == {n.split("<")[0] for n in cases.FOLLOW_KERNELS.values()}
    assert sorted(cases.FOLLOW_KERNELS) == list(range(1, 16))
    assert {v[3] for v in cases.FORMS.values()} == set(cases.FOLLOW_KERNELS)
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    listed = re.search(r"in this order from 1: (.*?) as 12\.\.15", header, re.S).group(1)
    names = re.findall(r"\b(\w+_kernel(?:_gated)?)\b", listed)
    assert names == [cases.FOLLOW_KERNELS[i] for i in range(1, 12)] + ["beam_ensemble_update_kernel"]


STEP_IDS = ["%s-%s" % (c.form, c.name) for c in cases.ALL_STEP_CASES]


@pytest.mark.parametrize("case", cases.ALL_STEP_CASES, ids=STEP_IDS)
def test_step_case_preconditions(case):
    inp, opts = cases.step_inputs(case), cases.rule_options(case)
    form, B, k, t, T, V = case.form, case.B, case.k, case.t, case.T, case.V
    W = 1 if t == 0 else k
    assert inp["logits"].shape == (cases.FORMS[form][1], B * W, V) and inp["hist_in"].shape == (B * W, T)
    assert 0 <= inp["hist_in"].min() and inp["hist_in"].max() < V                           # every index inside its table
    assert len(np.unique(inp["lp_in"])) == inp["lp_in"].size and len(np.unique(inp["anc_in"])) == inp["anc_in"].size
    assert len({tuple(r) for r in inp["hist_in"][:, :max(t, 1)].tolist()}) == B * W or t == 0   # distinct per row
    for name in ("ids", "words"):
        if name in opts:
            assert 0 <= opts[name].min() and opts[name].max() < V and len(opts[name]) == B
    if case.d_model is not None:
        assert all(w.shape == (V, d) and p.shape == (t + 3, d) and d % 4 == 0 for (w, p), d in zip(inp["emb"], case.d_model))
    M, ls = cases.host_pieces(inp["logits"])
    parents, words, scores, forced_images, _ = cases.winners(case, inp, opts, M, ls)
    assert parents.shape == words.shape == (B, k)
    assert 0 <= parents.min() and parents.max() < W and 0 <= words.min() and words.max() < V
    nan_image = 1 if case.nan else -1
    sampler = form in ("sample", "sample_shaped")
    for b in range(B):
        if b == nan_image or sampler:
            continue
        if form != "forced":
            assert np.isfinite(scores[b]).all(), "fewer than k finite candidates"
        if forced_images is not None and forced_images[b]:
            continue
        # no exact tie between winners of different rows: the order of equal scores is the selection's business, not this file's
        fin = np.isfinite(scores[b])
        for i in range(k):
            for j in range(i):
                assert not (fin[i] and fin[j] and scores[b, i] == scores[b, j] and parents[b, i] != parents[b, j]), (b, i, j)
    plain_rule = form in cases.COUNTING or form.startswith("ensemble")
    if plain_rule and W > 1 and not case.nan:
        assert parents[0].tolist() == list(range(k - 1, -1, -1))                            # a non-identity permutation
        if B > 1:
            assert set(parents[1].tolist()) == {min(2, W - 1)}                               # all the same row
        if B > 2 and W > 2:
            rows = 2 * W + parents[2]
            assert (inp["alive"][rows] == 0).any() and (words[2] == EOS).any() and (words[2] == cases.PAD).any()
            # a frozen parent in a slot that is not its row, under a live row of that number: the alive flag is the parent's
            assert any(inp["alive"][r] == 0 and inp["alive"][2 * W + j] != 0 for j, r in enumerate(rows))


def test_step_cases_cover_the_table():
    for form in cases.FORMS:
        mine = [c for c in cases.ALL_STEP_CASES if c.form == form]
        assert {c.t for c in mine} >= {0, 1, 255} and any(c.T == 256 and c.k * c.t > 512 for c in mine)
        sizes = {c.k * c.d_model[0] // 4 for c in mine if c.d_model}
        assert sizes >= ({1024, 4096, 1022, 1026} if form == "forced" else {1, 1023, 1024, 1025, 4096})
        assert any(c.nan for c in mine) and any(c.V == 16384 for c in mine)
        assert {c.V for c in mine} >= {33, 53, 1000}
        if form in cases.COUNTING:
            assert {c.B for c in mine if c.count and not c.nan and c.gate != 0} == {1, 3, 70}
        if cases.FORMS[form][2]:
            assert any(c.gate == 0 for c in mine) and any(c.gate == 1 for c in mine)
        if cases.FORMS[form][1] > 1:
            assert any(c.d_model and len(set(c.d_model)) > 1 for c in mine)                  # members of different widths

"""Inputs of ``tests/test_beam_state_gpu.py``: the case lists of the search's bookkeeping kernels (``csrc/beam.hip``) and their arrays,
from seeded generators.  No GPU here: ``tests/test_beam_state_cpu.py`` checks the lists and their preconditions.

Every array of a step case is generated for ``MAX_IMAGES`` images from one seeded generator per case; a launch over ``B`` images takes
the first ``B`` of them, so image 2 is the same image in a launch of 3 and in a launch of 9.
"""
import collections

import numpy as np

from openviic_amd import constraints, diverse, ensemble, forced, length, prefix, sampling

PAD, BOS, EOS, UNK = 0, 1, 2, 3
MAX_IMAGES = 9
F32 = np.float32

# The kernels of beam.hip that end in beam_follow_winners, by the id ovc_debug_beam_step returns (include/ovc.h), and the four
# instances of the ensemble kernel.  tests/test_beam_state_cpu.py holds this list to the source text.
FOLLOW_KERNELS = {
    1: "beam_update_kernel", 2: "beam_update_kernel_gated", 3: "beam_fused_update_kernel", 4: "beam_fused_update_kernel_gated",
    5: "beam_constrained_update_kernel", 6: "beam_prefix_update_kernel", 7: "beam_diverse_update_kernel", 8: "beam_forced_update_kernel",
    9: "beam_normalized_update_kernel", 10: "sample_fused_update_kernel", 11: "sample_shaped_update_kernel",
    12: "beam_ensemble_update_kernel<1>", 13: "beam_ensemble_update_kernel<2>", 14: "beam_ensemble_update_kernel<3>",
    15: "beam_ensemble_update_kernel<4>"}
FINAL_FORMS = ("plain", "gated", "forced", "normalized")

# form id -> (the entry's form code, members, gated, the kernel it must launch)
FORMS = collections.OrderedDict([
    ("two_pass", (6, 1, False, 1)), ("two_pass_gated", (6, 1, True, 2)), ("best", (0, 1, False, 3)), ("best_gated", (0, 1, True, 4)),
    ("constrained", (1, 1, False, 5)), ("prefix", (2, 1, False, 6)), ("diverse", (3, 1, False, 7)), ("forced", (4, 1, False, 8)),
    ("normalized", (5, 1, False, 9)), ("sample", (7, 1, False, 10)), ("sample_shaped", (8, 1, False, 11)),
    ("ensemble1", (9, 1, False, 12)), ("ensemble2", (9, 2, False, 13)), ("ensemble3", (9, 3, False, 14)), ("ensemble4", (9, 4, False, 15))])
COUNTING = ("best", "best_gated", "two_pass", "two_pass_gated")         # the forms that take alive_count

# name: what the case is for.  d_model: one width per member, or None (no next input rows).  gate: the gate word of a gated form.
StepCase = collections.namedtuple("StepCase", "name form B k t T V d_model nan count gate seed")

# k * d_model / 4 = the float4 of a step's next input rows: one pass of beam_follow_winners holds 1024
NEXT_X = ((1, 4), (3, 1364), (4, 1024), (5, 820), (8, 2048))            # 1, 1023, 1024, 1025, 4096
# The forced-word rule takes k in {2, 4, 8} only (2^C banks divide k), so 1, 1023 and 1025 float4 cannot be reached through it: it runs
# the passes on both sides of 1024 that it can reach, and 1024 and 4096 themselves
NEXT_X_FORCED = ((2, 4), (2, 2044), (4, 1024), (2, 2052), (8, 2048))    # 2, 1022, 1024, 1026, 4096


def _width_list(form, d):
    members = FORMS[form][1]
    return None if d is None else tuple([d] + [(64, 820, 12)[i] for i in range(members - 1)])


def step_cases(form):
    """The cases of one form: the three steps, the next_x passes, the NaN image, all 512 blocks, and for the counting forms the
    early-exit count at three batch sizes and the closed gate."""
    gated = FORMS[form][2]
    gate = 1 if gated else None
    kk = lambda k: max(2, k & ~1) if form == "forced" else k
    cases = [StepCase("t0", form, 3, kk(3), 0, 5, 53, _width_list(form, 64), False, False, gate, 11),
             StepCase("t1", form, 3, kk(3), 1, 6, 33, _width_list(form, 64), False, False, gate, 12),
             StepCase("tlast", form, 3, 8, 255, 256, 1000, None, False, False, gate, 13),
             StepCase("tmid", form, 3, 8, 200, 256, 1000, _width_list(form, 64), False, False, gate, 14),
             StepCase("nan", form, 3, kk(3), 2, 6, 53, _width_list(form, 64), True, form in COUNTING, gate, 15),
             StepCase("blocks512", form, 1, 4, 1, 4, 16384, _width_list(form, 8), False, False, gate, 16)]
    for i, (k, d) in enumerate(NEXT_X_FORCED if form == "forced" else NEXT_X):
        cases.append(StepCase("next_x_%d" % (k * d // 4), form, 3, k, 0 if k == 1 else 3, 7, 53, _width_list(form, d), False, False, gate, 20 + i))
    if form in COUNTING:
        for B in (1, 3, 70):
            cases.append(StepCase("count_B%d" % B, form, B, 3, 2, 6, 1000 if B == 70 else 33, None, False, True, gate, 30 + B))
    if gated:
        cases.append(StepCase("closed", form, 3, 3, 2, 6, 33, _width_list(form, 64), False, True, 0, 40))
    return cases


ALL_STEP_CASES = [c for form in FORMS for c in step_cases(form)]


def rule_options(case):
    """The rule's payload of a case, a dict of plain values and arrays (tables for B images)."""
    g = np.random.default_rng(1000 + case.seed)
    form, B, k, T, V, t = case.form, case.B, case.k, case.T, case.V, case.t
    nimg = max(MAX_IMAGES, B)                               # tables are drawn for every image and cut to the first B
    if form == "constrained":
        return {"ngram": 2, "min_length": min(t + 1, T - 1), "banned": sorted(int(w) for w in g.choice(np.arange(4, V), size=3, replace=False))}
    if form == "prefix":
        P = min(T - 1, 3)
        # per image: forced (while t < P), at its first free step, no prefix; a single image has no prefix
        lengths = np.array([(P, min(t, P), 0)[(b + (2 if B == 1 else 0)) % 3] for b in range(B)], np.int32)
        return {"P": P, "ids": g.integers(4, V, size=(nimg, P)).astype(np.int32)[:B], "lengths": lengths}
    if form == "diverse":
        return {"groups": k if k % 2 else 2, "diversity": 0.5}
    if form == "forced":
        C = 1 if k < 8 else 2
        return {"C": C, "words": np.stack([g.choice(np.arange(4, V), size=C, replace=False) for _ in range(nimg)]).astype(np.int32)[:B]}
    if form == "normalized":
        inv, bonus = length.tables(0.7, "wu", 0.1, T)
        return {"inv": inv, "bonus": bonus}
    if form == "sample":
        return {"seed": 0x1234567 + case.seed}
    return {}


def step_inputs(case):
    """The arrays of a case: ``logits [members][R][V]``, ``running / alive [R]``, ``hist_in / lp_in / anc_in [R][T]``, ``len_in [R]``,
    ``chosen [B*k]`` and the members' ``(word_emb [V][d], pos_emb [t + 3][d])``.

    Image 0's rows are peaked (one word each, far above the rest) with running scores that rise with the row, so its parents are the
    rows in reverse; image 1 has one row far ahead, so every parent is that row; image 2 has a frozen row that wins, a row whose best
    word is <eos> and one whose best is <pad>; the other images are random with frozen rows.  With ``nan`` image 1 holds NaN logits."""
    form, k, t, T, V = case.form, case.k, case.t, case.T, case.V
    members = FORMS[form][1]
    W = 1 if t == 0 else k
    g = np.random.default_rng(case.seed)
    nimg = max(MAX_IMAGES, case.B)
    R = nimg * W
    logits = (3.0 * g.standard_normal((members, R, V))).astype(F32)
    running = (-5.0 * g.random(R)).astype(F32)
    alive = np.ones(R, F32)
    peaked = form in ("sample", "sample_shaped")           # a sampler's word is unambiguous where one word holds all the mass
    if W > 1:
        alive[g.random(R) < 0.3] = 0
        alive[:3 * W] = 1
        if not peaked:
            words = g.choice(np.arange(4, V), size=W, replace=False)
            for i in range(W):                              # image 0: row i's best candidate scores 3 i, its second about -30
                logits[:, i, :] -= 30
                logits[:, i, words[i]] = 30
                running[i] = 3.0 * i - 3.0 * W
            lead = min(2, W - 1)                            # image 1: every winner from this row
            running[W:2 * W] = -100
            running[W + lead] = 0
            if nimg > 2:                                    # image 2: a frozen row ahead of all, <eos> and <pad> on top of two rows
                alive[2 * W + 1] = 0                        # (row 1 wins slot 0: the winner's slot is not its parent's row)
                running[2 * W + 1] = 1.0
                logits[:, 2 * W, EOS] = 12
                running[2 * W] = 0.5
                if W > 2:
                    logits[:, 2 * W + 2, PAD] = 12
                    running[2 * W + 2] = 0.25
    if peaked:
        top = g.integers(0, V, size=R)
        top[2 * W:3 * W] = ([EOS, PAD, V - 1, 31, 32, 5, 6, 7] * 2)[:W]
        logits[:, np.arange(R), top] = 60
        if W > 2:
            alive[2 * W + 2] = 0
    if case.nan:
        logits[:, W:2 * W, :] = np.nan
    # histories distinct per row in every column (among any V - 4 consecutive rows), with repeats inside a row
    r_, p_ = np.arange(R)[:, None], np.arange(T)[None, :]
    hist = (4 + (r_ + p_ * (5 + r_ % 3)) % (V - 4)).astype(np.int32)
    g.integers(4, V, size=(R, T))                          # (keeps the generator's position for what follows)
    inp = {"logits": logits, "running": running, "alive": alive,
           "hist_in": hist,
           "lp_in": (-(np.arange(R * T, dtype=np.float64).reshape(R, T) + 1) / 1024).astype(F32),
           "anc_in": (np.arange(R * T, dtype=np.int64).reshape(R, T) * 7 + 5).astype(np.int32),
           "len_in": np.where(alive != 0, t, g.integers(0, T + 6, size=R)).astype(np.int32),
           "chosen": g.integers(0, V, size=nimg * k).astype(np.int32)}
    inp["chosen"][:min(4, k)] = [EOS, PAD, V - 1, 32][:min(4, k)]
    if k > 1:
        inp["chosen"][k:k + 2] = [-3, V + 9]               # outside [0, V): the kernel clamps what it reads
    if case.d_model is not None:
        inp["emb"] = [((g.standard_normal((V, d))).astype(F32), (g.standard_normal((t + 3, d))).astype(F32)) for d in case.d_model]
    return take_images(inp, case.B, W, k)


def take_images(inp, B, W, k):
    """The first ``B`` images of every array."""
    out = dict(inp)
    out["logits"] = inp["logits"][:, :B * W]
    for n in ("running", "alive", "hist_in", "lp_in", "anc_in", "len_in"):
        out[n] = inp[n][:B * W]
    out["chosen"] = inp["chosen"][:B * k]
    return out


def host_pieces(logits):
    """``M`` and ``ls`` of every row in numpy: what the CPU checks feed the mirrors (the GPU tests feed them the entry's own)."""
    x = np.asarray(logits, F32)
    with np.errstate(invalid="ignore"):
        M = x.max(axis=-1)
        ls = np.log(np.exp((x - M[..., None]).astype(np.float64)).sum(axis=-1)).astype(F32)
    return M, ls


def winners(case, inp, opts, M, ls):
    """``(parents, words, scores, forced_images, extra)`` of a case from the package's mirrors of its rule, with the pieces ``M / ls
    [members][R]``.  Nothing is ranked here."""
    form, B, k, t, T = case.form, case.B, case.k, case.t, case.T
    W = 1 if t == 0 else k
    x, run, alive = inp["logits"], inp["running"], inp["alive"]
    none = np.zeros(B, np.int32)
    if form in COUNTING:
        return prefix.mirror_update(x[0], run, alive, k, t, None, none, M[0], ls[0]) + (None, None)
    if form == "constrained":
        banned = x[0].copy()                               # a banned word scores -inf under the plain rule: (-inf - M) - ls
        for r in range(B * W):
            if alive[r] != 0:
                for w in constraints.banned_at(inp["hist_in"][r], t, opts["ngram"], opts["min_length"], opts["banned"], EOS):
                    banned[r, w] = -np.inf
        return prefix.mirror_update(banned, run, alive, k, t, None, none, M[0], ls[0]) + (None, None)
    if form == "prefix":
        return prefix.mirror_update(x[0], run, alive, k, t, opts["ids"], opts["lengths"], M[0], ls[0]) + (t < opts["lengths"], None)
    if form == "diverse":
        return diverse.mirror_update(x[0], run, alive, k, opts["groups"], F32(opts["diversity"]), t, M[0], ls[0]) + (None, None)
    if form == "forced":
        return forced.mirror_update(x[0], run, alive, k, opts["words"], t, M[0], ls[0], PAD) + (None, None)
    if form == "normalized":
        p, w, raws, lens, keys = length.mirror_update(x[0], run, alive, inp["len_in"], k, t, M[0], ls[0], opts["inv"], opts["bonus"])
        return p, w, raws, None, {"len_out": lens, "key_out": keys}
    if form.startswith("ensemble"):
        p, w, s, _ = ensemble.mirror_update(x, M, ls, run, alive, k, t)
        return p, w, s, None, None
    # the samplers: slot s continues row s (the image's one row at step 0); a frozen row takes word 0
    parents = np.tile(np.arange(k) if W > 1 else np.zeros(k, np.int64), (B, 1))
    words = np.zeros((B, k), np.int64)
    u = sampling.uniforms(opts["seed"], B, k, t + 1)[:, :, t] if form == "sample" else None
    for b in range(B):
        for s in range(k):
            r = b * W + parents[b, s]
            if alive[r] == 0:
                continue
            if form == "sample":
                logp = (x[0][r].astype(np.float64) - np.float64(M[0][r])) - np.float64(ls[0][r])
                words[b, s] = sampling.mirror_sample(logp, u[b, s])
            else:
                words[b, s] = min(max(int(inp["chosen"][b * k + s]), 0), case.V - 1)
    return parents, words, np.zeros((B, k), F32), None, None


# ---- the final orderings ----------------------------------------------------------------------------------------------------------
FinalCase = collections.namedtuple("FinalCase", "name form k out_size T plant steps_run counts C seed")
FINAL_SIZES = [(k, o, T) for k in (1, 3, 8) for o in sorted({1, k}) for T in (1, 6, 65, 256)]
PLANTS = ("random", "pair", "equal", "neginf")        # an exact tie of two slots; all scores equal; -inf scores, one image of only -inf


def final_cases():
    cases = []
    for i, (k, o, T) in enumerate(FINAL_SIZES):
        plant = PLANTS[i % 4]
        cases.append(FinalCase("plain", "plain", k, o, T, plant, (0, 1, T - 1)[i % 3] if T > 1 else 0, None, None, 100 + i))
        cases.append(FinalCase("normalized", "normalized", k, o, T, PLANTS[(i + 1) % 4], 0, None, None, 200 + i))
        cases.append(FinalCase("gated", "gated", k, o, T, PLANTS[(i + 2) % 4], 0, ("first", "none")[i % 2], None, 300 + i))
    for p, plant in enumerate(PLANTS):
        cases.append(FinalCase("plain_" + plant, "plain", 8, 8, 65, plant, (0, 1, 64, 0)[p], None, None, 400 + p))
        cases.append(FinalCase("gated_" + plant, "gated", 8, 8, 130, plant, 0, ("lanes", "first", "none", "lanes")[p], None, 410 + p))
        cases.append(FinalCase("normalized_" + plant, "normalized", 8, 8, 65, plant, 0, None, None, 420 + p))
        for k, C in ((2, 1), (8, 2), (8, 3)):
            cases.append(FinalCase("forced_%d_%d_%s" % (k, C, plant), "forced", k, (1, k)[p % 2], (6, 65, 256, 1)[p], plant, 0, None, C,
                                   430 + 10 * p + C))
    cases.append(FinalCase("normalized_keys", "normalized", 8, 8, 6, "keys", 0, None, None, 500))
    return cases


FINAL_CASES = final_cases()


def final_inputs(case, B=3):
    """``running [B*k]``, ``hist / lp [B*k][T]`` (and a second state of other data for the gated form), ``alive_count [T]``, ``len_in``,
    ``inv / bonus``.  No score is NaN: no search hands the plain, gated or forced ordering one (tests/test_beam_state_gpu.py)."""
    g = np.random.default_rng(case.seed)
    k, T = case.k, case.T
    R = B * k
    run = (-10.0 * g.random(R)).astype(F32)
    if case.plant == "pair" and k > 1:
        run[k - 1] = run[0]                                # image 0: the first and the last slot tie exactly
        run[k + 1:2 * k] = run[k]                          # image 1: every slot but ... all equal
    if case.plant == "equal":
        run[:] = F32(-2.5)
    if case.plant == "neginf":
        run[:k] = -np.inf                                  # image 0: no winner at all: slot order
        run[k::2] = -np.inf                                # the others: every second slot
    inp = {"running": run, "hist": g.integers(0, 1000, size=(R, T)).astype(np.int32), "lp": (-g.random((R, T))).astype(F32),
           "running2": run.reshape(B, k)[:, ::-1].reshape(-1).copy(), "hist2": g.integers(0, 1000, size=(R, T)).astype(np.int32), "lp2": (-g.random((R, T))).astype(F32)}
    counts = g.integers(1, 9, size=T).astype(np.int32)
    if case.counts == "first":
        counts[0] = 0
    if case.counts == "lanes":
        counts[70] = counts[100] = 0
    inp["alive_count"] = counts
    inp["len_in"] = g.integers(1, T + 1, size=R).astype(np.int32)
    inp["len_in"][0], inp["len_in"][R - 1] = 0, T + 5      # clamped to 1 and to T
    inp["inv"], inp["bonus"] = (np.array(a, F32) for a in length.tables(0.7, "wu", 0.1, T))
    if case.plant == "keys":
        # image 0: one length for all, so equal raw scores are equal keys and the slot decides; image 1: a bonus that absorbs every
        # raw score (1e9 + raw rounds to 1e9), so all keys are equal and the raw score decides; image 2: a NaN key, which comes last
        inp["len_in"][:] = 3
        run[1] = run[5]
        inp["len_in"][k:2 * k] = 2
        inp["bonus"][1], inp["inv"][1] = 1e9, 1.0
        run[2 * k + 3] = np.nan
    return inp

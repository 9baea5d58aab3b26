"""The scope of every training sizer, pinned: what each of the twelve training sizers and the dropout search's sizer answers for
a fixed set of hand-built descriptors and shapes is recorded in ``golden/train_scope.json`` (from the library of the commit before
the scope predicates became one function) and must stay equal, byte for byte -- a zero is a refusal; every refused cell's entry
point refuses too, before any pointer is read; and the host's architecture table names exactly the library's entry points (no
GPU needed).

The shapes ``(B, N, T, S)`` are the smallest that reach every branch of the limits, worked out from the predicates' formulas for
the descriptors' V = 10201, d = 512, d_ff = 2048, max_len = 20 (K = 2^31 - 1 - 2^20, the 32-bit descriptor bound):

* ``(V + 256) * pad4(rows) * 4 <= K``: rows <= 51312 -- ``(51312, 1, 1, 1)`` is accepted, ``(51313, 1, 1, 1)`` refused;
* ``(rows + 256) * pad4(V) * 4 <= K``: rows <= 52332.  For every vocabulary the fused tail takes (V <= 16384 < sqrt(K)) the
  term above refuses first, so no shape fails this one alone: ``(52333, 1, 1, 1)`` fails both;
* the stacked rows, ``(factor * max(rows, B*N) + 256) * 2048 * 4 <= K``, i.e. factor * max(rows, B*N) <= 261759: three levels
  (meshed) accept ``(43626, 2, 1, 1)`` and refuse ``(43627, 2, 1, 1)``; factor 1 (AoA) accepts ``(255, 1024, 1, 1)`` and
  refuses ``(256, 1024, 1, 1)`` -- every other scope accepts all four;
* ``4 d^2 * 4 <= K`` (AoA) holds for every d_model <= 2048 a model may have: no descriptor reaches it;
* N <= 1024 (the box-relation backward, and every pass) and T <= max_len: ``(4, 1024, 20, 5)`` / ``(4, 1025, 20, 5)`` and
  ``(4, 50, 21, 5)``.

``PYTHONPATH=. python tests/test_train_scope_cpu.py`` (with ``OVC_LIBRARY`` naming the library to record from) rewrites the fixture."""
import ctypes
import json
import os

import pytest

from helpers import GOLDEN
from openviic_amd import native, train_arch
from test_aoa_train_cpu import aoa_desc, gate, plain_desc
from test_camo_cpu import _camo_desc
from test_geometric_train_cpu import geometric_desc
from test_memory_train_cpu import memory_desc
from test_meshed_train_cpu import meshed_desc

FIXTURE = os.path.join(GOLDEN, "train_scope.json")
FAKE = 4096
EINVAL = -1

SHAPES = [(4, 50, 20, 5), (1, 1, 1, 1), (3, 129, 7, 2),
          (51312, 1, 1, 1), (51313, 1, 1, 1), (52333, 1, 1, 1),
          (43626, 2, 1, 1), (43627, 2, 1, 1), (255, 1024, 1, 1), (256, 1024, 1, 1),
          (4, 1024, 20, 5), (4, 1025, 20, 5), (4, 50, 21, 5)]


def _half(site, **missing):
    d = aoa_desc()
    gate({"enc": d.enc[0].att, "self": d.dec[2].self_att, "cross": d.dec[1].cross_att}[site], **missing)
    return d


DESCRIPTORS = {
    "plain": plain_desc,
    "plain_v16384": lambda: plain_desc(vocab=16384),            # either side of the fused vocabulary tail's limit
    "plain_v16385": lambda: plain_desc(vocab=16385),
    "camo": _camo_desc,
    "memory": memory_desc,
    "meshed": meshed_desc,
    "meshed_no_memory": lambda: meshed_desc(memory=0),
    "geometric_trig": geometric_desc,
    "geometric_plain": lambda: geometric_desc(False),
    "aoa_all": aoa_desc,
    "aoa_enc": lambda: aoa_desc("enc"),
    "aoa_cross": lambda: aoa_desc("cross"),
    "aoa_enc_without_sigmoid_gate": lambda: _half("enc", g=False),
    "aoa_self_without_informative_gate": lambda: _half("self", i=False),
    "aoa_cross_without_informative_gate": lambda: _half("cross", i=False),
}

P = ctypes.c_void_p(FAKE)
BIG = 1 << 40


def _loss_entry(name, *tail):
    return lambda lib, d, B, N, T, S: getattr(lib, name)(ctypes.byref(d), ctypes.byref(d), P, P, B, N, P, P, T, P, BIG, P, 0, None, *tail)


def _sequence_entry(name, *tail):
    return lambda lib, d, B, N, T, S: getattr(lib, name)(ctypes.byref(d), ctypes.byref(d), P, P, B, N, S, P, P, T, P, BIG, None, 0,
                                                          None, *tail)


def _drop():
    return ctypes.byref(native.Dropout(seed=FAKE))


def _cells():
    """cell -> (sizer symbol, its arguments behind the model from (B, N, T, S), the entry point's call with fake pointers)."""
    cells = {
        "train": ("ovc_train_workspace_bytes", lambda B, N, T, S: (B, N, T), _loss_entry("ovc_forward_backward")),
        "dropout": ("ovc_train_dropout_workspace_bytes", lambda B, N, T, S: (B, N, T),
                    _loss_entry("ovc_forward_backward_dropout", _drop())),
        "beams": ("ovc_train_beams_workspace_bytes", lambda B, N, T, S: (B, N, S, T), _sequence_entry("ovc_sequence_backward")),
        "beams_dropout": ("ovc_train_beams_dropout_workspace_bytes", lambda B, N, T, S: (B, N, S, T),
                          _sequence_entry("ovc_sequence_backward_dropout", 5, P, _drop())),
        "search_dropout": ("ovc_beam_search_dropout_workspace_bytes", lambda B, N, T, S: (B, N, S),
                           lambda lib, d, B, N, T, S: lib.ovc_beam_search_dropout(ctypes.byref(d), P, P, B, N, S, 1, P, BIG, P, P, None,
                                                                                  _drop(), P, 0, None, None)),
    }
    for flag in (0, 1):
        drop = _drop() if flag else None
        args = lambda B, N, T, S, flag=flag: (B, N, T, flag)
        cells["smoothed/%d" % flag] = ("ovc_train_smoothed_workspace_bytes", args, _loss_entry(
            "ovc_forward_backward_smoothed", ctypes.byref(native.Loss(0.1, native.LOSS_REDUCTIONS["mean"])), drop))
        cells["distill/%d" % flag] = ("ovc_train_distill_workspace_bytes", args, _loss_entry(
            "ovc_forward_backward_distill", ctypes.byref(native.Distill(FAKE, 0.5)), drop))
    for arch in train_arch.TRAIN_ARCHS.values():
        for flag in (0, 1) if arch.loss_dropout else (None,):
            tail = () if flag is None else (_drop() if flag else None,)
            cells[arch.key if flag is None else "%s/%d" % (arch.key, flag)] = (
                arch.loss_form[0], lambda B, N, T, S, flag=flag: (B, N, T) if flag is None else (B, N, T, flag),
                _loss_entry(arch.loss_form[1], *tail))
        cells[arch.key + "_beams"] = (arch.sequence_form[0], lambda B, N, T, S: (B, N, S, T), _sequence_entry(arch.sequence_form[1]))
    return cells


CELLS = _cells()


def _key(shape):
    return "B{}_N{}_T{}_S{}".format(*shape)


def measure(lib):
    return {name: {_key(shape): {cell: getattr(lib, sizer)(ctypes.byref(d), *args(*shape)) for cell, (sizer, args, _) in CELLS.items()}
                   for shape in SHAPES}
            for name, d in ((name, make()) for name, make in DESCRIPTORS.items())}


@pytest.fixture(scope="module")
def recorded():
    """The fixture holds one row of bytes per descriptor and shape, in the order of its ``cells`` list."""
    with open(FIXTURE) as f:
        table = json.load(f)
    return {name: {shape: dict(zip(table["cells"], row)) for shape, row in shapes.items()} for name, shapes in table["bytes"].items()}


def write_fixture(measured, path):
    cells = list(CELLS)
    rows = ",\n".join('  "{}": {{\n{}\n  }}'.format(name, ",\n".join(
        '   "{}": {}'.format(shape, json.dumps([row[c] for c in cells])) for shape, row in shapes.items()))
        for name, shapes in measured.items())
    with open(path, "w") as out:
        out.write('{{\n "cells": {},\n "bytes": {{\n{}\n }}\n}}\n'.format(json.dumps(cells), rows))


def test_the_table_covers_every_training_sizer_once():
    sizers = {sizer for sizer, _, _ in CELLS.values()}
    named = {n for n in native.SIGNATURES if n.startswith("ovc_train_") and n.endswith("_workspace_bytes")}
    assert sizers == named | {"ovc_beam_search_dropout_workspace_bytes"} and len(sizers) == 13


def test_every_sizer_answers_the_recorded_bytes(recorded):
    got = measure(native.load())
    assert set(got) == set(recorded)
    for name in got:
        assert got[name] == recorded[name], (name, {s: {c: (v, recorded[name][s][c]) for c, v in row.items() if v != recorded[name][s][c]}
                                                   for s, row in got[name].items() if row != recorded[name][s]})
    # the draw is not vacuous: every cell is accepted somewhere and refused somewhere, every limit shape on both sides
    for cell in CELLS:
        answers = [row[cell] for shapes in recorded.values() for row in shapes.values()]
        assert any(answers) and not all(answers), cell
    assert recorded["plain"][_key((51312, 1, 1, 1))]["train"] > 0 == recorded["plain"][_key((51313, 1, 1, 1))]["train"]
    assert recorded["meshed"][_key((43626, 2, 1, 1))]["meshed"] > 0 == recorded["meshed"][_key((43627, 2, 1, 1))]["meshed"]
    assert recorded["aoa_all"][_key((255, 1024, 1, 1))]["aoa/0"] > 0 == recorded["aoa_all"][_key((256, 1024, 1, 1))]["aoa/0"]
    assert recorded["plain"][_key((256, 1024, 1, 1))]["train"] > 0 and recorded["plain"][_key((43627, 2, 1, 1))]["train"] > 0
    assert recorded["geometric_trig"][_key((4, 1024, 20, 5))]["geometric/1"] > 0 == recorded["geometric_trig"][_key((4, 1025, 20, 5))]["geometric/1"]
    assert recorded["plain_v16384"][_key((4, 50, 20, 5))]["train"] > 0 == recorded["plain_v16385"][_key((4, 50, 20, 5))]["train"]


def test_every_refused_cell_is_refused_by_its_entry_point(recorded):
    """Only refused cells are called: an accepted one would go on to the device."""
    lib = native.load()
    called = 0
    for name, make in DESCRIPTORS.items():
        d = make()
        for shape in SHAPES:
            for cell, (_, _, entry) in CELLS.items():
                if recorded[name][_key(shape)][cell] == 0:
                    assert entry(lib, d, *shape) == EINVAL, (name, shape, cell)
                    called += 1
    assert called > 1000


def test_the_host_table_names_the_library_entry_points():
    for key, arch in train_arch.TRAIN_ARCHS.items():
        assert arch.key == key
        mine = {n for n in native.SIGNATURES if n.endswith("_" + key) or "_{}_".format(key) in n and "debug" not in n}
        assert mine == {*arch.loss_form, *arch.sequence_form}, key
        (sizer, entry), (seq_sizer, seq_entry) = arch.loss_form, arch.sequence_form
        assert sizer.startswith("ovc_train_") and entry.startswith("ovc_forward_backward_")
        assert seq_sizer.endswith("_beams_workspace_bytes") and seq_entry.startswith("ovc_sequence_backward_")
        # the loss form takes the dropout flag / table exactly where the table says so
        assert len(native.SIGNATURES[sizer][1]) == (5 if arch.loss_dropout else 4)
        assert (native.SIGNATURES[entry][1][-1] == ctypes.POINTER(native.Dropout)) == arch.loss_dropout
        assert train_arch.of_variant(arch.variant) is arch and train_arch.resolve(**{key: True}) is arch
    assert set(train_arch.TRAIN_ARCHS) == {"meshed", "geometric", "aoa"}
    assert train_arch.resolve() is None and train_arch.of_variant("standard_transformer") is None
    assert [a.key for a in train_arch.TRAIN_ARCHS.values() if a.needs_boxes] == ["geometric"]


def test_two_keywords_name_two_different_models():
    for keywords, text in ((dict(meshed=True, geometric=True), "meshed=True and geometric=True"),
                           (dict(aoa=True, meshed=True), "aoa=True and meshed=True"),
                           (dict(aoa=True, geometric=True), "aoa=True and geometric=True"),
                           (dict(aoa=True, meshed=True, geometric=True), "meshed=True and geometric=True")):
        with pytest.raises(native.OvcError) as raised:
            train_arch.resolve(**keywords)
        assert str(raised.value) == text + " name two different models: pass the one this model is"


if __name__ == "__main__":
    write_fixture(measure(native.load()), FIXTURE)
    print("recorded", FIXTURE, "from", native.LIBRARY_PATH)

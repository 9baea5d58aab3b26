"""The training architectures that are reached through a keyword of their own (``meshed=True`` / ``geometric=True`` /
``aoa=True``), each described once: ``engine.py`` takes the entry points and the engine-level refusals from an entry,
``architectures.py`` the refusals of ``xe_loss`` / ``xe_step`` / ``scst_step`` / ``beam_search``, the probes under ``tools/`` the
keyword and the sizer.  ``None`` stands for the models the plain entry points train (the standard, augmented-memory and CaMo
transformers); the device side's ``TrainArch`` (``csrc/engine.hip``) is the same list."""
from dataclasses import dataclass

from .native import OvcError


@dataclass(frozen=True)
class TrainArch:
    key: str                # the public keyword
    noun: str               # the model's name in messages
    variant: str            # the configuration that builds it (``config.model_config``)
    loss_form: tuple        # (sizer, entry point) of the loss form ...
    sequence_form: tuple    # ... and of the sequence form
    loss_dropout: bool      # the loss form takes the dropout table (or NULL) behind the plain arguments, its sizer the flag
    dropout_note: str       # what a refusal of ``dropout`` adds (``refuse_with``)
    needs_boxes: bool = False
    # (sizer, entry point) of the loss form under dropout where the plain loss form takes none: reached through
    # ``dropout=LEVEL_DROPOUT`` -- one module applied once per encoder level, a mask per level (``openviic_amd.dropout``)
    level_dropout_form: tuple = None
    # the SCST pair under dropout, reached through ``dropout=BEAM_LEVEL_DROPOUT``: (sizer, entry point) of the search and of the
    # sequence form's recompute -- the level-keyed mask at the search's mask row (``openviic_amd.dropout``)
    beam_level_search_form: tuple = None
    beam_level_sequence_form: tuple = None

    def keywords(self):
        return {self.key: True}

    def takes_level_dropout(self, dropout):
        """``dropout`` is the level-keyed spelling and this architecture has that form."""
        return self.level_dropout_form is not None and isinstance(dropout, str) and dropout == LEVEL_DROPOUT

    def takes_beam_level_dropout(self, dropout):
        """``dropout`` is the SCST spelling of the level-keyed form and this architecture has it."""
        return self.beam_level_search_form is not None and isinstance(dropout, str) and dropout == BEAM_LEVEL_DROPOUT

    def refuse_in_engine(self, where, dropout, loss=False, distill=False):
        """What ``forward_backward`` / ``sequence_backward`` (``where``) refuse together with this architecture: the smoothed
        loss and soft targets always, dropout where the loss form has none and in the sequence form."""
        if where == "sequence_backward":
            if dropout:
                raise OvcError("sequence_backward({}=True): {} is out of scope for {}".format(
                    self.key, "the sequence form under dropout" if self.loss_dropout else "dropout", self.noun))
        elif loss or distill or (dropout and not self.loss_dropout):
            raise OvcError("forward_backward({}=True): {}the label-smoothed loss and soft targets are out of scope for {}".format(
                self.key, "" if self.loss_dropout else "dropout, ", self.noun))

    def refuse_with(self, what, **given):
        """This architecture's keyword together with what its training does not cover, another architecture's keyword among
        it: the first of ``given`` that is set is refused by name."""
        for name, value in given.items():
            if value and name != self.key:
                raise OvcError("{}({}=True, {}=...): {} is out of scope for {}'s training{}".format(
                    what, self.key, name, name, self.noun,
                    self.dropout_note if name == "dropout" else " -- a model is one or the other" if name in TRAIN_ARCHS else ""))


LEVEL_DROPOUT = "levels"    # ``xe_loss`` / ``xe_step``'s ``dropout`` value that selects an architecture's ``level_dropout_form``
# ``beam_search`` / ``scst_step``'s ``dropout`` value that selects an architecture's ``beam_level_search_form`` / ``..._sequence_form``
BEAM_LEVEL_DROPOUT = "beam_levels"

_SEARCH_HAS_ITS_OWN_SCOPE = " -- the search under dropout has its own scope; set DROPOUT: 0 or call model.eval()"

TRAIN_ARCHS = {a.key: a for a in (
    TrainArch("meshed", "the meshed-memory transformer", "meshed_memory_transformer",
              ("ovc_train_meshed_workspace_bytes", "ovc_forward_backward_meshed"),
              ("ovc_train_meshed_beams_workspace_bytes", "ovc_sequence_backward_meshed"), loss_dropout=False,
              dropout_note=" -- the meshed layer applies enc_attn.dropout once per level, with a mask per level: xe_loss / xe_step take "
                           "dropout=\"levels\" for it, beam_search / scst_step dropout=\"beam_levels\"; or set DROPOUT: 0 or call "
                           "model.eval()",
              level_dropout_form=("ovc_level_dropout_workspace_bytes", "ovc_forward_backward_level_dropout"),
              beam_level_search_form=("ovc_beam_search_level_dropout_workspace_bytes", "ovc_beam_search_level_dropout"),
              beam_level_sequence_form=("ovc_level_dropout_beams_workspace_bytes", "ovc_sequence_backward_level_dropout")),
    TrainArch("geometric", "the object-relation transformer", "object_relation_transformer",
              ("ovc_train_geometric_workspace_bytes", "ovc_forward_backward_geometric"),
              ("ovc_train_geometric_beams_workspace_bytes", "ovc_sequence_backward_geometric"), loss_dropout=True,
              dropout_note=_SEARCH_HAS_ITS_OWN_SCOPE, needs_boxes=True),
    TrainArch("aoa", "the attention-on-attention transformer", "attention_on_attention",
              ("ovc_train_aoa_workspace_bytes", "ovc_forward_backward_aoa"),
              ("ovc_train_aoa_beams_workspace_bytes", "ovc_sequence_backward_aoa"), loss_dropout=True,
              dropout_note=_SEARCH_HAS_ITS_OWN_SCOPE),
)}


def named(**keywords):
    """The architectures whose keyword is set, in the order the keywords are given: a caller's refusals fire in that order."""
    return [TRAIN_ARCHS[key] for key, value in keywords.items() if value]


def resolve(meshed=False, geometric=False, aoa=False):
    """The three public keywords as ``None`` or one ``TrainArch``; two of them together name two different models."""
    given = named(geometric=geometric, meshed=meshed, aoa=aoa)
    if len(given) > 1:      # the later keyword of the pair first: meshed and geometric; aoa and either
        raise OvcError("{}=True and {}=True name two different models: pass the one this model is".format(given[1].key, given[0].key))
    return given[0] if given else None


def of_variant(variant):
    """The architecture a configuration builds, or ``None``."""
    return next((a for a in TRAIN_ARCHS.values() if a.variant == variant), None)

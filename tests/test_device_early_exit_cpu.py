"""Device-side early exit (ovc_beam_search_gated) without a GPU: the C entry point is declared, bound and exported, and the
host accepts exactly the early-exit values it documents."""
import ctypes
import os
import re

import pytest

from openviic_amd import native
from openviic_amd.engine import CaptionEngine, _early_exit_from_env, early_exit_mode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gated_search_is_declared_bound_and_exported():
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        header = f.read()
    decl = re.search(r"int ovc_beam_search_gated\(([^;]*)\);", header)
    assert decl, "ovc_beam_search_gated is not declared in include/ovc.h"
    assert "int32_t* steps_out" in decl.group(1) and "ovc_stream stream" in decl.group(1)
    restype, argtypes = native.SIGNATURES["ovc_beam_search_gated"]
    assert len(argtypes) == 13 and argtypes[0] == native.SIGNATURES["ovc_beam_search_early"][1][0]
    lib = native.load()
    assert hasattr(lib, "ovc_beam_search_gated")
    assert lib.ovc_abi_version() == 8


def test_gated_search_refuses_bad_arguments_before_touching_a_device():
    lib = native.load()
    # a null model (and null buffers) is refused with OVC_EINVAL before any device call
    assert lib.ovc_beam_search_gated(None, None, None, 1, 1, 1, 1, None, 0, None, None, None, None) == -1      # OVC_EINVAL


def test_every_search_refuses_null_arguments_before_touching_a_device():
    """All five search entry points go through one front end: a null model and null buffers are OVC_EINVAL (-1) there, and
    ovc_beam_search_dropout's own checks (a null table, a mode outside 0..2) come first."""
    lib = native.load()
    head = (None, None, None, 1, 1, 1, 1, None, 0, None, None)     # model, features, boxes, B, N, k, out_size, workspace, bytes, ids, logp
    assert lib.ovc_beam_search(*head, None, None) == -1
    assert lib.ovc_beam_search_graph(*head, None) == -1
    assert lib.ovc_beam_search_early(*head, None, None) == -1
    assert lib.ovc_beam_search_gated(*head, None, None) == -1
    slots = (ctypes.c_int32 * 1)()
    for mode in (0, 1, 2):
        assert lib.ovc_beam_search_dropout(*head, None, None, None, mode, None, None) == -1
        assert lib.ovc_beam_search_dropout(*head, None, None, slots, mode, None, None) == -1            # a null dropout table
    assert lib.ovc_beam_search_dropout(*head, None, None, None, 3, None, None) == -1


@pytest.mark.parametrize("value,mode", [(None, False), (False, False), (True, True), ("device", "device")])
def test_early_exit_values(value, mode):
    assert early_exit_mode(value) is mode if not isinstance(mode, str) else early_exit_mode(value) == mode


@pytest.mark.parametrize("value", ["host", "1", 1, 0, "Device", 2.0, [], "true"])
def test_other_early_exit_values_are_refused(value):
    with pytest.raises(native.OvcError, match="early_exit"):
        early_exit_mode(value)


def test_environment_switch():
    assert _early_exit_from_env("0") is False
    assert _early_exit_from_env("1") is True
    assert _early_exit_from_env("device") == "device"
    assert CaptionEngine.early_exit in (False, True, "device")

"""Device-side early exit (ovc_beam_search_gated) without a GPU: the C entry point is declared, bound and exported, and the
host accepts exactly the early-exit values it documents."""
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

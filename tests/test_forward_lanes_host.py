"""Option "forward_lanes" (two working sets and two internal streams per handle, csrc/model.hip: fwd_route) on the host:
its validation, its environment variable and its text in the header.  The GPU side is tests/test_gpu_forward_lanes.py.

vk_option_check and vk_option_default are host-only entry points: vk_set_option validates through the first, and
vk_create takes every option's starting value from the second."""
import ctypes as C
import os
import re

import pytest

from vltk_amd import _lib as L

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def default(key):
    v = C.c_int(-1)
    L.call("vk_option_default", key.encode(), C.byref(v))
    return v.value


def test_forward_lanes_takes_one_or_two():
    lib = L.load()
    for v in (1, 2):
        assert lib.vk_option_check(b"forward_lanes", v) == L.VK_OK
    for v in (0, 3, -1):
        assert lib.vk_option_check(b"forward_lanes", v) == L.VK_EINVAL
        assert b"forward_lanes must be 1 or 2" in lib.vk_last_error()
    with pytest.raises(ValueError, match="forward_lanes must be 1 or 2"):
        L.call("vk_option_check", b"forward_lanes", 3)
    assert lib.vk_option_check(b"forward_lane", 1) == L.VK_EINVAL          # an unknown key


def test_set_option_validates_through_option_check():
    """One copy of the rules: vk_set_option calls vk_option_check before it stores anything, and the other options keep
    their ranges."""
    src = open(os.path.join(ROOT, "vltk_amd", "csrc", "model.hip")).read()
    body = src[src.index("int vk_set_option("):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"VK_TRY\(vk_option_check\(key, value\)\);", body)
    stores = [m.start() for m in re.finditer(r"h->[^;=]*=(?!=)", body)]       # every store through the handle, whichever option
    assert stores and body.index("VK_TRY(vk_option_check(key, value));") < min(stores)
    assert not re.search(r"\bif\b|\bstrcmp\b", body)      # no per-option branch: the one store serves every key of the table
    lib = L.load()
    for key, good, bad in ((b"backbone_streams", (1, 4), (0, 5)), (b"head_streams", (1, 2), (0, 3)), (b"head_chunk", (0, 9600), (-1,)),
                           (b"head_split_min_rois", (2,), (1,)), (b"backbone_split_min_batch", (2,), (1,))):
        assert all(lib.vk_option_check(key, v) == L.VK_OK for v in good), key
        assert all(lib.vk_option_check(key, v) == L.VK_EINVAL for v in bad), key


def test_environment_variable_is_parsed(monkeypatch):
    monkeypatch.delenv("VK_FORWARD_LANES", raising=False)
    assert default("forward_lanes") == 2
    for text, want in (("1", 1), ("2", 2), ("0", 2), ("3", 2), ("", 2), ("two", 2), ("1x", 2), ("12", 2)):
        monkeypatch.setenv("VK_FORWARD_LANES", text)
        assert default("forward_lanes") == want, text
    monkeypatch.delenv("VK_FORWARD_LANES")
    # the variables that were there before keep their meaning
    monkeypatch.delenv("VK_BACKBONE_STREAMS", raising=False)
    monkeypatch.delenv("VK_HEAD_STREAMS", raising=False)
    monkeypatch.delenv("VK_HEAD_CHUNK", raising=False)
    assert (default("backbone_streams"), default("head_streams"), default("head_chunk")) == (2, 1, 9600)
    monkeypatch.setenv("VK_BACKBONE_STREAMS", "3")
    monkeypatch.setenv("VK_HEAD_STREAMS", "2")
    monkeypatch.setenv("VK_HEAD_CHUNK", "4800")
    assert (default("backbone_streams"), default("head_streams"), default("head_chunk")) == (3, 2, 4800)
    monkeypatch.setenv("VK_HEAD_CHUNK", "0")
    assert default("head_chunk") == 9600
    # ... and their parsing: the first digit of the stream counts, atoi of the chunk
    monkeypatch.setenv("VK_BACKBONE_STREAMS", "3x")
    monkeypatch.setenv("VK_HEAD_STREAMS", "12")
    monkeypatch.setenv("VK_HEAD_CHUNK", "4800abc")
    assert (default("backbone_streams"), default("head_streams"), default("head_chunk")) == (3, 1, 4800)
    monkeypatch.setenv("VK_BACKBONE_STREAMS", "5")
    monkeypatch.setenv("VK_HEAD_STREAMS", "3")
    assert (default("backbone_streams"), default("head_streams")) == (2, 1)


def test_create_reads_the_defaults_from_option_default():
    src = open(os.path.join(ROOT, "vltk_amd", "csrc", "model.hip")).read()
    body = src[src.index("int vk_create("):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"for \(const OptionRow &o : kOptions\) \(void\)vk_option_default\(o\.key, &\(h->\*o\.member\)\);", body)
    assert "getenv(\"VK_FORWARD_LANES\")" not in body
    # no option's variable is read here: every VK_* name in the option table, and VK_PREDICTOR_FP16 (an A/B switch) may stay
    table = src[src.index("kOptions[] = {"):]
    table = table[:table.index("\n};\n")]
    variables = re.findall(r'"(VK_[A-Z_]+)"', table)
    assert len(variables) == 5 and "VK_FORWARD_LANES" in variables, variables
    for v in variables:
        assert v not in body, v
    assert set(re.findall(r'getenv\("(\w+)"\)', body)) <= {"VK_PREDICTOR_FP16"}


def test_header_documents_the_option_and_the_buffer_lifetime():
    header = open(os.path.join(ROOT, "include", "vltk_hip.h")).read()
    text = " ".join(header.split())
    assert '"forward_lanes"' in text and "VK_FORWARD_LANES" in text
    opts = text[text.index("/* Tunables."):text.index("int vk_set_option(")]
    for key in ('"backbone_streams"', '"head_streams"', '"forward_lanes"'):      # documented side by side
        assert key in opts, key
    begin = text[text.index("The same forward in two halves"):text.index("int vk_forward_begin(")]
    assert "must not be written, freed or reused" in begin and "Until _end of its ticket" in begin

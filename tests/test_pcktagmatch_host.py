"""What of the tag matcher's packed-index entry point (include/gtamd_pcktag.h)
can be checked without a device: the header against the binding, the library
without a fallback, and the recorded outputs of the reference."""
import hashlib
import json
import os
import re

import pytest

import oracle_util as ou
from genometools_amd import _lib, tagmatch

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_pcktag.h")


def test_every_declared_symbol_is_exported_and_bound():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(gtamd_[a-z_0-9]+)\s*\(", text)))
    assert declared == ["gtamd_tagmatch_set_index_pckidx"] == sorted(_lib.PCKTAG_ABI)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.PCKTAG_ABI[name][1], name
        assert getattr(lib, name).restype == _lib.PCKTAG_ABI[name][0], name
    assert HEADER in _lib.HEADERS
    assert os.path.join(_lib.HERE, "csrc", "esa_pckidx_dec.h") in _lib.HEADERS
    assert hasattr(tagmatch.TagMatches, "set_index_packed")
    # the header is a layer over the two it joins and adds no type of its own
    assert '#include "gtamd_pckidx.h"' in text and '#include "gtamd_tagmatch.h"' in text and "typedef" not in text


def test_no_cpu_fallback():
    lib = _lib.load()
    if lib.gtamd_device_count() > 0:
        pytest.skip("a device is present")
    # neither a matcher nor a reader is to be had: the call has nothing to work on
    assert not lib.gtamd_tagmatch_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    assert not lib.gtamd_pckidx_create(0)
    assert b"no HIP device" in lib.gtamd_esa_last_error()
    assert lib.gtamd_tagmatch_set_index_pckidx(None, None) == -1
    assert b"invalid argument to gtamd_tagmatch_set_index_pckidx" in lib.gtamd_esa_last_error()


def test_the_recorded_outputs_are_those_of_the_json():
    with open(os.path.join(ou.GOLDEN_DIR, "golden_pcktagmatch.json")) as f:
        golden = json.load(f)
    with open(os.path.join(ou.GOLDEN_DIR, "golden_tagmatch.json")) as f:
        esa_calls = json.load(f)["calls"]
    assert len(golden["texts"]) == 3
    for name, key in golden["texts"].items():
        with open(os.path.join(ou.GOLDEN_DIR, "pcktagmatch", name), "rb") as f:
            raw = f.read()
        want = golden["calls"][key]
        assert (hashlib.md5(raw).hexdigest(), raw.count(b"\n")) == (want["md5"], want["lines"])
    # every call is one of the suffix-table recording, and "as_esa" says what it says
    for key, entry in list(golden["calls"].items()) + list(golden["wildcard_calls"].items()):
        other = esa_calls[key.rsplit("|", 1)[0]]
        assert entry["as_esa"] == ((entry["md5"], entry["exit"]) == (other["md5"], other["exit"])), key
        assert ("-withwildcards" in key) == (key in golden["wildcard_calls"])
    with open(os.path.join(ou.GOLDEN_DIR, "pcktagmatch", golden["image"][2]), "rb") as f:
        from genometools_amd import pck
        pck.check_image(f.read())

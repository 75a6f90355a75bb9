"""What of the aligner's packed-index entry point (include/gtamd_pcklocali.h) can
be checked without a device: the header as plain C, the header against the
binding, the library without a fallback."""
import os
import re
import subprocess

from genometools_amd import _lib, locali

HEADER = os.path.join(_lib.ROOT, "include", "gtamd_pcklocali.h")


def test_the_header_is_plain_c(tmp_path):
    source = tmp_path / "use.c"
    source.write_text('#include "gtamd_pcklocali.h"\n'
                      "int use(gtamd_locali *lc, const gtamd_pckidx *px) { return gtamd_locali_set_index_pckidx(lc, px); }\n")
    for std in ("-std=c99", "-std=c11"):
        subprocess.run(["cc", std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.dirname(HEADER), "-c",
                        str(source), "-o", str(tmp_path / "use.o")], check=True)


def test_every_declared_symbol_is_exported_and_bound():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = _lib.load()
    declared = sorted(set(re.findall(r"\b(gtamd_[a-z_0-9]+)\s*\(", text)))
    assert declared == ["gtamd_locali_set_index_pckidx"] == sorted(_lib.PCKLOCALI_ABI)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.PCKLOCALI_ABI[name][1], name
        assert getattr(lib, name).restype == _lib.PCKLOCALI_ABI[name][0], name
    assert HEADER in _lib.HEADERS
    assert hasattr(locali.LocalAlignments, "set_index_packed")
    # the header is a layer over the two it joins and adds no type of its own
    assert '#include "gtamd_pckidx.h"' in text and '#include "gtamd_locali.h"' in text and "typedef" not in text


def test_no_cpu_fallback():
    """Without a device neither an aligner nor a reader can be created, so the null
    arguments are the only path of the entry point that can be reached: -1 and its
    message.  The missing device itself shows in the two create calls."""
    lib = _lib.load()
    assert lib.gtamd_locali_set_index_pckidx(None, None) == -1
    assert b"invalid argument to gtamd_locali_set_index_pckidx" in lib.gtamd_esa_last_error()
    if lib.gtamd_device_count() == 0:
        # neither an aligner nor a reader is to be had: the call has nothing to work on
        assert not lib.gtamd_locali_create(0)
        assert b"no HIP device" in lib.gtamd_esa_last_error()
        assert not lib.gtamd_pckidx_create(0)
        assert b"no HIP device" in lib.gtamd_esa_last_error()

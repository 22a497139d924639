"""The gate of exec mode 'auto' for the one-launch streaming decode batch, without a GPU:
clay_amd.DECODE_STREAM_BATCH_AUTO_MAX_SC restates kDecodeStreamBatchMaxSc of engine.hip, the
docstrings name it, and the new translation unit is in every link list of the Makefile."""
import os
import re

import clay_amd
from clay_amd import ClayCode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clay_amd", "csrc")


def test_python_constant_restates_the_engine_gate():
    src = open(os.path.join(CSRC, "engine.hip")).read()
    m = re.findall(r"constexpr size_t kDecodeStreamBatchMaxSc = (\d+);", src)
    assert len(m) == 1, m
    assert int(m[0]) == clay_amd.DECODE_STREAM_BATCH_AUTO_MAX_SC
    assert "DECODE_STREAM_BATCH_AUTO_MAX_SC" in clay_amd.__all__
    # a closed gate is documented as unmeasured; an open one cites its sweep
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    if clay_amd.DECODE_STREAM_BATCH_AUTO_MAX_SC == 0:
        assert "batch_decode_stream_gate" in design and "unmeasured" in design
    else:
        assert "profiles/r14/batch_decode_stream_gate.txt" in design
        assert f"{clay_amd.DECODE_STREAM_BATCH_AUTO_MAX_SC:,}" in design


def test_interface_text_names_the_path():
    for doc in (clay_amd.set_exec_mode.__doc__, clay_amd.last_exec_path.__doc__,
                ClayCode.decode_device_strided.__doc__):
        assert "stream-local256-batch" in doc
    assert "streaming batch" in ClayCode.decode_device_batch.__doc__
    hdr = open(os.path.join(ROOT, "include", "clay.h")).read()
    assert "stream-local256-batch" in hdr


def test_new_unit_is_in_every_link_list():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    lists = [line for line in mk.splitlines() if "decode_local256_any.o" in line and ":" in line.split("decode_local256_any.o")[0]
             and not line.startswith(("build/decode_local256_any.o", "build/asan/decode_local256_any.o"))]
    assert len(lists) == 3, lists  # OBJS, the asan library, the probe library
    for line in lists:
        assert "decode_local256_batch.o" in line, line
    assert "decode_local256_batch.hip" in [w for line in mk.splitlines() if line.startswith("SRCS") for w in line.split()]
    assert "decode-batch-res:" in mk

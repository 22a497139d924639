"""The batch of the fused decode v2 ("stream-fused2-batch") without a GPU: the gate of exec mode
'auto' (clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC restates kDecodeFused2BatchMaxSc of engine.hip and
follows from the committed sweep by the stated rule), the interface text names the path, the new
translation unit is in every link list of the Makefile, and the patterns of the GPU tests are what
those tests say they are."""
import json
import os
import re

import clay_amd
import decode_pattern
from clay_amd import ClayCode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clay_amd", "csrc")
SWEEP = os.path.join(ROOT, "profiles", "r15", "batch_decode_fused2_gate.txt")


def test_python_constant_restates_the_engine_gate():
    src = open(os.path.join(CSRC, "engine.hip")).read()
    m = re.findall(r"constexpr size_t kDecodeFused2BatchMaxSc = (\d+);", src)
    assert len(m) == 1, m
    assert int(m[0]) == clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC
    assert "DECODE_FUSED2_BATCH_AUTO_MAX_SC" in clay_amd.__all__
    # a closed gate is documented as unmeasured or with what was measured; an open one cites its sweep
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "batch_decode_fused2_gate" in design
    if clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC:
        assert "profiles/r15/batch_decode_fused2_gate.txt" in design
        assert f"{clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC:,}" in design


def test_gate_follows_from_the_committed_sweep():
    """The rule: the largest swept sub-chunk up to which the batch's median is at most the loop's
    plus the spread (max - min) of the loop's samples in every cell; 0 when there is no sweep or
    the smallest sub-chunk already fails."""
    if not os.path.exists(SWEEP):
        assert clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC == 0
        return
    cells = [json.loads(line) for line in open(SWEEP) if line.startswith("{")]
    assert cells
    ok = {}
    for c in cells:
        sc = int(re.search(r"\(sc (\d+)\)", c["config"]).group(1))
        assert c["batch"]["path"] == "stream-fused2-batch" and c["batch"]["launches"] == 1, c["config"]
        assert c["loop"]["path"] == "stream-fused2", c["config"]
        fine = c["batch"]["median_us"] <= c["loop"]["median_us"] + c["loop"]["spread_us"]
        assert fine == c["batch_no_slower"], c["config"]
        ok[sc] = ok.get(sc, True) and fine
    gate = 0
    for sc in sorted(ok):
        if not ok[sc]:
            break
        gate = sc
    assert clay_amd.DECODE_FUSED2_BATCH_AUTO_MAX_SC == gate, (gate, ok)


def test_interface_text_names_the_path():
    for doc in (clay_amd.set_exec_mode.__doc__, clay_amd.last_exec_path.__doc__,
                ClayCode.decode_device_strided.__doc__, ClayCode.decode_device_batch.__doc__):
        assert "stream-fused2-batch" in doc
    for doc in (clay_amd.set_exec_mode.__doc__, ClayCode.decode_device_strided.__doc__):
        assert "DECODE_FUSED2_BATCH_AUTO_MAX_SC" in doc
    hdr = open(os.path.join(ROOT, "include", "clay.h")).read()
    assert "stream-fused2-batch" in hdr and "kDecodeFused2BatchMaxSc" in hdr


def test_new_unit_is_in_every_link_list():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    lists = [line for line in mk.splitlines() if "decode_local256_any.o" in line and ":" in line.split("decode_local256_any.o")[0]
             and not line.startswith(("build/decode_local256_any.o", "build/asan/decode_local256_any.o"))]
    assert len(lists) == 3, lists  # OBJS, the asan library, the probe library
    for line in lists:
        assert "decode_fused2_batch.o" in line, line
    assert "decode_fused2_batch.hip" in [w for line in mk.splitlines() if line.startswith("SRCS") for w in line.split()]
    assert "build/asan/decode_fused2_batch.o:" in mk and "fused2-batch-res:" in mk


def test_gpu_test_patterns_are_what_the_cases_say():
    """tests/test_gpu_decode_batch_fused2.py's patterns run on k_stream_fused2 under "stream": four on
    the plain instantiation, four on TWO with (2,1,1), (2,2), (2,1,1) and (2,1,1) sections, and the
    last has a split step (DecArgs::split, decode_pattern.fused2_args)."""
    from test_gpu_decode_batch_fused2 import PATTERNS
    c = decode_pattern.code(10)
    two, split = [], []
    for er in PATTERNS:
        assert decode_pattern.expected_kernel(c, list(er), "stream") == "fused2", er
        two.append(max(decode_pattern.per_section(c, er)) == 2)
        split.append(decode_pattern.fused2_args(c, list(er))[1])
    assert two == [False, False, False, False, True, True, True, True]
    assert [sorted(decode_pattern.per_section(c, er)) for er in PATTERNS[4:]] == \
        [[0, 1, 1, 2], [0, 0, 2, 2], [0, 1, 1, 2], [0, 1, 1, 2]]
    assert split[:7] == [0] * 7 and split[7] != 0, split

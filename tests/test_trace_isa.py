"""CPU: the gfx950 code of the benchmark's traversal kernel, trace_kernel_coop<float, false, true, 0, false> (closest hit, robust,
triangles, quad-cooperative record fetch), compiled here by hipcc with the library's own flags (bvh_amd/build.py) to assembly.
Guards what the instruction stream of its inner-node loop relies on: 8 waves per SIMD (at most 64 VGPRs), no scratch beyond the
stack's spill array and the few spills it has always had, and four record loads that no lane guard splits (trace_device.h:
coop_load_pair: a lane that wants no record reads zeros beyond the buffer's end instead of branching around its load)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from bvh_amd import build as bvh_build

KERNEL = "_ZN7bvh_amd12_GLOBAL__N_117trace_kernel_coopIfLb0ELb1ELi0ELb0EEEvNS0_9TraceArgsIT_EE"
MAX_SCRATCH = 208          # bytes per lane before the unconditional fetch: the 44-entry spill array (176) + two 8-byte spills


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(bvh_build.HIPCC):
        pytest.fail(f"hipcc not found at {bvh_build.HIPCC}")
    out = str(tmp_path_factory.mktemp("isa") / "traverse.s")
    src = os.path.join(ROOT, "bvh_amd", "csrc", "traverse.hip")
    r = subprocess.run([bvh_build.HIPCC] + bvh_build.FLAGS + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read().splitlines()


def _kernel(lines):
    i = next(k for k, line in enumerate(lines) if line.startswith(KERNEL + ":"))
    j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
    meta = {}
    for line in lines[j:j + 80]:
        m = re.match(r"\s*;\s*(NumVgprs|ScratchSize|Occupancy):\s*(\d+)", line)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    return lines[i:j], meta


def _inner_loop(body):
    """Instructions of the depth-2 loop that holds the quad transpose (the inner-node loop), as [(block label, [instructions])] in layout
    order, the loop header first. Loop membership comes from the loop annotations LLVM writes beside each block label ("Loop Header:
    Depth=2", "in Loop: Header=BBx_y Depth=2"): if a compiler update changes that format, this fails loudly instead of passing."""
    blocks = []
    for line in body:
        m = re.match(r"^(\.LBB\w+):\s*(.*)$", line)
        if m:
            blocks.append([m.group(1), m.group(2), []])
            continue
        if not blocks:
            continue
        text = line.split(";")[0].strip()
        if not text and line.strip().startswith(";") and not blocks[-1][2]:
            blocks[-1][1] += " " + line.strip()          # the loop annotations continue on comment lines under the label
        elif text and not text.startswith("."):
            blocks[-1][2].append(text)
    loops = {}
    for label, note, ins in blocks:
        m = re.search(r"Header=BB(\w+) Depth=2", note)
        if m:
            loops.setdefault(".LBB" + m.group(1), []).append((label, ins))
        elif "Loop Header: Depth=2" in note:
            loops.setdefault(label, []).append((label, ins))
    for header, members in loops.items():
        if any("_dpp" in t for _, ins in members for t in ins):
            k = next(i for i, (label, _) in enumerate(members) if label == header)
            return members[k:] + members[:k]
    raise AssertionError("no inner loop with the DPP transpose in " + KERNEL)


def test_bench_kernel_registers_and_scratch(asm):
    _, meta = _kernel(asm)
    assert meta["NumVgprs"] <= 64, meta
    assert meta["Occupancy"] >= 8, meta
    assert meta["ScratchSize"] <= MAX_SCRATCH, meta


def test_record_loads_unguarded(asm):
    body, _ = _kernel(asm)
    loop = _inner_loop(body)
    where = [(b, k) for b, (_, ins) in enumerate(loop) for k, t in enumerate(ins) if t.startswith("buffer_load_dwordx4")]
    assert len(where) == 4, f"expected the four record loads of coop_load_pair, found {len(where)}"
    assert len({b for b, _ in where}) == 1, "the record loads are spread over several basic blocks"
    # from the loop header to the last record load: no lane guard of any kind, in the loads' block or in a block before it
    b, k = where[-1]
    path = [t for _, ins in loop[:b] for t in ins] + loop[b][1][:k + 1]
    guards = [t for t in path if re.match(r"s_(and|or|xor|andn2|orn2)_saveexec|s_cbranch_exec|s_\w+_b64\s+exec", t)]
    assert not guards, guards
    assert not any(t.startswith("global_load") for _, ins in loop for t in ins), "a record load left the buffer path"

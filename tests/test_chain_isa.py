"""The hand-off of the chained kernels, checked in the gfx950 code of the built library (no GPU needed).

Disassembles drl-tetris_amd/lib/libtetris_hip.so with the ROCm llvm-objdump (skips when the tool or the library is missing,
fails when a library that exists cannot be unpacked) and checks:
- k_chain_affine<1>, k_chain<1>: the epoch poll is wave-uniform (it branches on scalar conditions, with no exec-mask
  bookkeeping), and no wait for a scalar load lies between it and the state loads: the row stride is read before the poll;
- k_chain_affine<1>, k_duo_affine: the flag words in host memory that they write (F_PLACE, F_XCC0) are system-scope vector
  stores, and no wait for them follows before the wave branches or ends;
- k_chain_affine<1>, k_duo_affine: the epoch publication is the one store after the final drain of the wave's stores, a plain
  global store (the line stays in the XCD's L2), with no wait behind it.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "drl-tetris_amd", "lib", "libtetris_hip.so")
F_PLACE, F_XCC0 = 6, 8           # csrc/tetris_layout.h (te::Flag)
STATE_LOADS = 27                 # words a single-player step loads (tetris_engine.h: load_game)
# program order from the poll loop's first branch to the first state load: the rest of the loop and the rarely taken give-up
# path lie in between (the taken path, a match at the first poll, runs 26 of them); a guard against growth, not the path length
MAX_POLL_TO_LOAD = 160


def _objdump():
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump"), shutil.which("llvm-objdump")):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tool = _objdump()
    if tool is None:
        pytest.skip("llvm-objdump of ROCm not found")
    if not os.path.exists(LIB):
        pytest.skip("libtetris_hip.so not built")
    d = tmp_path_factory.mktemp("isa")
    lib = os.path.join(str(d), "lib.so")
    shutil.copy(LIB, lib)
    r = subprocess.run([tool, "--offloading", lib], capture_output=True, text=True, cwd=str(d))
    assert r.returncode == 0, f"llvm-objdump --offloading failed on the built library: {r.stderr[-300:]}"
    text = ""
    for f in sorted(os.listdir(str(d))):
        if "gfx950" in f:
            text += subprocess.run([tool, "-d", "--demangle", os.path.join(str(d), f)], capture_output=True, text=True, check=True).stdout
    funcs, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
        if m:
            name = m.group(2)
            funcs[name] = []
        elif name and line.startswith("\t"):
            ins, _, comment = line.strip().partition("//")
            addr = re.match(r"\s*([0-9A-F]+):", comment)
            funcs[name].append((int(addr.group(1), 16) if addr else None, ins.strip()))
    return funcs


def _body(funcs, name):
    for k, v in funcs.items():
        if k.startswith(name + "("):
            return v
    pytest.fail(f"{name} not found in the disassembly")


@pytest.mark.parametrize("name", ["void k_chain_affine<1>", "void k_chain<1>"])
def test_poll_is_uniform_and_no_scalar_wait_precedes_the_state_loads(kernels, name):
    ins = [i for _, i in _body(kernels, name)]
    # the poll: an `sc1` load of the epoch word whose value is made wave-uniform right away ...
    poll = next(k for k, i in enumerate(ins) if re.match(r"global_load_dword v\d+, v\d+, s\[\d+:\d+\] sc1$", i)
                and any(j.startswith("v_readfirstlane_b32") for j in ins[k + 1:k + 8]))
    # ... and the loop decides on scalar conditions: its first branch tests SCC or VCC, no exec mask is saved before it
    br = next(k for k in range(poll + 1, len(ins)) if ins[k].startswith(("s_cbranch", "s_branch")))
    assert ins[br].startswith(("s_cbranch_scc", "s_cbranch_vcc")), f"{name}: the poll's exit is not a uniform branch: {ins[br]}"
    assert not any("saveexec" in i for i in ins[poll:br]), f"{name}: exec-mask bookkeeping in the poll"
    # the block that issues the 27 state loads of a single-player step (from the branch before the first one) waits for no
    # scalar load: the kernel arguments it needs were read before the poll
    loads = [k for k in range(br, len(ins)) if ins[k].startswith("buffer_load_dword")][:STATE_LOADS]
    assert len(loads) == STATE_LOADS, f"{name}: fewer than {STATE_LOADS} state loads after the poll"
    start = max(k for k in range(br, loads[0]) if ins[k].startswith(("s_cbranch", "s_branch")))
    assert not any(i.startswith(("s_cbranch", "s_branch")) for i in ins[start + 1:loads[-1]]), f"{name}: the state loads are not one block"
    waits = [i for i in ins[start + 1:loads[-1]] if i.startswith("s_waitcnt") and "lgkmcnt" in i]
    assert not waits, f"{name}: a wait for a scalar load among the state loads: {waits}"
    assert loads[0] - br <= MAX_POLL_TO_LOAD, f"{name}: {loads[0] - br} instructions between the poll's branch and the first state load"


AFFINE = ["void k_chain_affine<1>", "k_duo_affine"]
VMEM_STORE = re.compile(r"(global|flat|buffer)_(store|atomic)")


def _flag_pair(ins):
    # the status pointer: the base of the F_PLACE store (every affine kernel has one, on its misplaced-workgroup path)
    m = next(re.match(r"global_store_dword v\d+, v\d+, (s\[\d+:\d+\]) offset:%d sc0 sc1$" % (F_PLACE * 4), i) for i in ins
             if re.match(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\] offset:%d sc0 sc1$" % (F_PLACE * 4), i))
    return m.group(1)


@pytest.mark.parametrize("name", AFFINE)
def test_affine_flag_stores_do_not_wait(kernels, name):
    ins = [i for _, i in _body(kernels, name)]
    flag = [k for k, i in enumerate(ins) if re.match(rf"(global|flat)_store_dword .* offset:({F_PLACE * 4}|{F_XCC0 * 4}) ", i + " ")]
    assert flag, "no F_PLACE / F_XCC0 store found"
    for k in flag:
        assert ins[k].startswith("global_store_dword") and ins[k].endswith("sc0 sc1"), f"{name}: not a system-scope global store: {ins[k]}"
        for j in ins[k + 1:]:
            if j.startswith(("s_branch", "s_cbranch", "s_endpgm")):
                break
            assert "vmcnt(0)" not in j, f"{name}: a wait follows the flag store {ins[k]}"


@pytest.mark.parametrize("name", AFFINE)
def test_affine_epoch_publication_is_a_plain_store_after_the_drain(kernels, name):
    ins = [i for _, i in _body(kernels, name)]
    status = _flag_pair(ins)
    # every vector store the kernel makes outside the status words and the census marker (offset:128 = chain + CHAIN_STRIDE)
    # are state stores (buffer), counter atomics and the publication: exactly one global store is left
    pubs = [k for k, i in enumerate(ins) if i.startswith("global_store_dword") and status not in i and "offset:128" not in i]
    assert len(pubs) == 1, f"{name}: expected one epoch publication, found:\n" + "\n".join(ins[k] for k in pubs)
    k = pubs[0]
    assert re.match(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\]$", ins[k]), f"{name}: the publication is not a plain store: {ins[k]}"
    drain = max(j for j in range(k) if ins[j].startswith("s_waitcnt") and "vmcnt(0)" in ins[j])
    assert not any(VMEM_STORE.match(j) for j in ins[drain + 1:k]), f"{name}: a store between the final drain and the publication"
    assert any(j.startswith("buffer_store_dword") for j in ins[:drain]), f"{name}: no state store before the drain"
    assert "vmcnt(0)" not in ins[k + 1], f"{name}: a wait follows the publication"

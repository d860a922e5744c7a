"""The single-step chained kernels, checked in the gfx950 code of the built library (no GPU needed).

k_chain_affine<1> and k_chain<1> make one env-step per launch: csrc/tetris_hip.hip calls rollout_step once between the state
loads and the state stores, with no loop over a step count around it (launches of another step count run k_chain_fused*).
Disassembles drl-tetris_amd/lib/libtetris_hip.so with the ROCm llvm-objdump (skips when the tool or the library is missing) and
checks, for both kernels:
- no branch between the first state load and the last state store goes back to an address before that first load: inner
  loops of the step are allowed, a loop that encloses the step is not;
- the VGPR count of the kernel's metadata is no higher than 112, what the kernels needed with the loop around the step, and
  nothing is spilled (no scratch, no SGPR spills into VGPR lanes);
- no `s_mul_i32` lies between the first and the last state load, nor between the first and the last state store: the rows' byte
  offsets are multiplied out once, before the poll (tetris_engine.h: RowTable), and both the loads and the stores reuse them;
- the fused kernels exist beside them.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "drl-tetris_amd", "lib", "libtetris_hip.so")
STATE_LOADS = 27                 # words a single-player step loads (tetris_engine.h: load_game)
MAX_VGPRS = 112                  # k_chain_affine<1> / k_chain<1> with game_run's loop around the step
SINGLE = [("void k_chain_affine<1>", "_Z14k_chain_affineILi1EEvN2te5KArgsE"), ("void k_chain<1>", "_Z7k_chainILi1EEvN2te5KArgsE")]
FUSED = [("void k_chain_fused_affine<1>", "_Z20k_chain_fused_affineILi1EEvN2te5KArgsE"), ("void k_chain_fused<1>", "_Z13k_chain_fusedILi1EEvN2te5KArgsE")]


def _tool(name):
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name), shutil.which(name)):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def code(tmp_path_factory):
    """-> (funcs: demangled name -> [(address, instruction)], meta: mangled kernel name -> {key: int})"""
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    if objdump is None or readelf is None:
        pytest.skip("llvm-objdump / llvm-readelf of ROCm not found")
    if not os.path.exists(LIB):
        pytest.skip("libtetris_hip.so not built")
    d = tmp_path_factory.mktemp("isa_single")
    lib = os.path.join(str(d), "lib.so")
    shutil.copy(LIB, lib)
    r = subprocess.run([objdump, "--offloading", lib], capture_output=True, text=True, cwd=str(d))
    assert r.returncode == 0, f"llvm-objdump --offloading failed on the built library: {r.stderr[-300:]}"
    text, notes = "", ""
    for f in sorted(os.listdir(str(d))):
        if "gfx950" in f:
            text += subprocess.run([objdump, "-d", "--demangle", os.path.join(str(d), f)], capture_output=True, text=True, check=True).stdout
            notes += subprocess.run([readelf, "--notes", os.path.join(str(d), f)], capture_output=True, text=True, check=True).stdout
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
    # the kernels' metadata (amdhsa.kernels): the keys of an entry come in alphabetical order, `.name` before the counts read here
    meta, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "name" and m.group(2).startswith("_Z"):
            cur = meta.setdefault(m.group(2), {})
        elif m.group(1) == "agpr_count":
            cur = None
        elif cur is not None and m.group(1) in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            cur[m.group(1)] = int(m.group(2))
    return funcs, meta


def _body(funcs, name):
    for k, v in funcs.items():
        if k.startswith(name + "("):
            return v
    pytest.fail(f"{name} not found in the disassembly")


def _step_range(body, name):
    """indices of the first state load and of the last state store"""
    ins = [i for _, i in body]
    # the poll: an `sc1` load of the epoch word made wave-uniform right away; the state loads are the buffer loads behind its exit
    poll = next(k for k, i in enumerate(ins) if re.match(r"global_load_dword v\d+, v\d+, s\[\d+:\d+\] sc1$", i)
                and any(j.startswith("v_readfirstlane_b32") for j in ins[k + 1:k + 8]))
    loads = [k for k in range(poll, len(ins)) if ins[k].startswith("buffer_load_dword")][:STATE_LOADS]
    assert len(loads) == STATE_LOADS, f"{name}: fewer than {STATE_LOADS} state loads after the poll"
    stores = [k for k in range(loads[-1], len(ins)) if ins[k].startswith("buffer_store_dword")]
    assert len(stores) >= STATE_LOADS, f"{name}: fewer than {STATE_LOADS} state stores behind the loads"
    return loads, stores


@pytest.mark.parametrize("name,mangled", SINGLE)
def test_no_loop_encloses_the_step(code, name, mangled):
    funcs, _ = code
    body = _body(funcs, name)
    loads, stores = _step_range(body, name)
    first_addr = body[loads[0]][0]
    assert first_addr is not None
    back = []
    for addr, ins in body[loads[0]:stores[-1] + 1]:
        m = re.match(r"s_c?branch\w*\s+(\d+)$", ins)
        if not m or addr is None:
            continue
        simm = int(m.group(1))
        simm -= 0x10000 if simm >= 0x8000 else 0
        target = addr + 4 + 4 * simm
        if target < first_addr:
            back.append(f"{addr:x}: {ins} -> {target:x}")
    assert not back, f"{name}: a branch inside the step goes back in front of the first state load ({first_addr:x}):\n" + "\n".join(back)


@pytest.mark.parametrize("name,mangled", SINGLE)
def test_registers_no_higher_than_with_the_loop_and_nothing_spilled(code, name, mangled):
    funcs, meta = code
    assert mangled in meta, f"{mangled} not found in the kernels' metadata"
    m = meta[mangled]
    print(f"{name}: {m}")
    assert m["vgpr_count"] <= MAX_VGPRS, f"{name}: {m['vgpr_count']} VGPRs"
    assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0 and m.get("private_segment_fixed_size", 0) == 0, f"{name}: {m}"
    assert not [i for _, i in _body(funcs, name) if i.startswith(("v_writelane", "scratch_"))], f"{name}: spill code in the kernel"


@pytest.mark.parametrize("name,mangled", SINGLE)
def test_no_row_offset_multiply_among_the_state_loads_or_stores(code, name, mangled):
    funcs, _ = code
    body = _body(funcs, name)
    loads, stores = _step_range(body, name)
    ins = [i for _, i in body]
    for what, lo, hi in (("loads", loads[0], loads[-1]), ("stores", stores[0], stores[-1])):
        muls = [f"{k}: {ins[k]}" for k in range(lo, hi + 1) if ins[k].startswith("s_mul_i32")]
        assert not muls, f"{name}: scalar multiplies among the state {what}:\n" + "\n".join(muls)


@pytest.mark.parametrize("name,mangled", FUSED)
def test_fused_kernels_exist_and_use_no_scratch(code, name, mangled):
    funcs, meta = code
    _body(funcs, name)
    assert mangled in meta, f"{mangled} not found in the kernels' metadata"
    assert meta[mangled].get("private_segment_fixed_size", 0) == 0       # (direct dispatch refuses kernels with scratch)

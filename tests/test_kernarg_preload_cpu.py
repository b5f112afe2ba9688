"""CPU-only checks of the decode kernels' entry (magpie-tts.cpp_amd/Makefile,
-amdgpu-kernarg-preload-count; mp_decode.hip, gemv_kernel's note): the decode
kernels take their entry path's scalars as leading arguments, which gfx950's command
processor places in SGPRs at wave start, so the first loads wait for no scalar load.

Read from the built library, the way test_layout_abi_cpu.py gets its code objects:
 - every such kernel's descriptor asks for a non-zero kernarg preload length;
 - from the real entry point (256 bytes in: the block before it reloads the arguments
   for firmware that does not preload them) to the first global_load there is no
   s_waitcnt on lgkmcnt, except the profiling stamp's own (the wait that follows
   s_memrealtime in ts_begin, on a path taken only while a launch is being profiled).
A build that loses the flag, or a kernel change that puts a struct field in front of the
first loads, fails here."""
import re
import struct
import subprocess

from test_layout_abi_cpu import _gfx950_code_objects

LLVM = "/opt/rocm/lib/llvm/bin/"
# the f32 family's decode kernels, by their mangled names' stems
KERNELS = ("N2mp11gemv_kernelI", "N2mp14lt_ffn2_kernelI", "N2mp15lt_front_kernelE", "N2mp18lt_finalize_kernelE",
           # the 16-bit and Q8_0 families' decode kernels
           "N2mp15gemm_b16_kernelI", "N2mp18gemm_q8_kernel_decI", "N2mp14lt_slot_kernelE", "N2mp17lt_slot_q8_kernelI")
# instantiation counts a library must at least hold (the fused GEMV family is instantiated
# for batches 1, 2, 4, 8 and a few ops at 16; lt_ffn2 for 1, 2, 4, 8)
MIN_COUNT = {"N2mp11gemv_kernelI": 60, "N2mp14lt_ffn2_kernelI": 4, "N2mp15lt_front_kernelE": 1,
             "N2mp18lt_finalize_kernelE": 1, "N2mp15gemm_b16_kernelI": 60, "N2mp18gemm_q8_kernel_decI": 40,
             "N2mp14lt_slot_kernelE": 1, "N2mp17lt_slot_q8_kernelI": 4}


def _sections_and_symbols(co):
    """({section index: (address, file offset)}, {symbol: (value, section index, size)}) of an ELF64 code object"""
    data = co.read_bytes()
    assert data[:4] == b"\x7fELF" and data[4] == 2, "ELF64"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = []
    for i in range(shnum):
        _, typ, _, addr, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize)
        secs.append((typ, addr, off, size, link, entsize))
    syms = {}
    for typ, _, off, size, link, entsize in secs:
        if typ != 2:  # SHT_SYMTAB
            continue
        stroff = secs[link][2]
        for k in range(size // entsize):
            name, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", data, off + k * entsize)
            end = data.index(b"\0", stroff + name)
            syms[data[stroff + name:end].decode()] = (value, shndx, size)
    return data, {i: (s[1], s[2]) for i, s in enumerate(secs)}, syms


def _instructions(co):
    """[(address, text)] of the code object's disassembly, in address order"""
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--mcpu=gfx950", str(co)], capture_output=True, text=True,
                         check=True).stdout
    out = []
    for m in re.finditer(r"^\s+(\S[^\n]*?)\s*// ([0-9A-Fa-f]+):", dis, re.M):
        out.append((int(m.group(2), 16), m.group(1)))
    return out


def test_decode_kernels_preload_their_entry_scalars(tmp_path):
    import bisect
    import magpie_amd as ma
    found = {k: 0 for k in KERNELS}
    bad = []
    for co in _gfx950_code_objects(ma.LIB_PATH, tmp_path):
        data, secs, syms = _sections_and_symbols(co)
        names = [s for s in syms if s + ".kd" in syms and any(k in s for k in KERNELS)]
        if not names:
            continue
        ins = _instructions(co)
        addrs = [a for a, _ in ins]
        for name in names:
            found[next(k for k in KERNELS if k in name)] += 1
            # kernel descriptor (64 bytes): KERNARG_PRELOAD_SPEC_LENGTH is bits 464..470
            value, shndx, _ = syms[name + ".kd"]
            kd = data[value - secs[shndx][0] + secs[shndx][1]:][:64]
            length = struct.unpack_from("<H", kd, 58)[0] & 0x7F
            if length == 0:
                bad.append(f"{name}: kernarg preload length 0 (built without the preload flag, or no leading scalars)")
                continue
            # the real entry, behind the 256-byte block that reloads the arguments
            entry = syms[name][0] + 256
            i = bisect.bisect_left(addrs, entry)
            assert i < len(ins) and addrs[i] == entry, f"{name}: no instruction at entry + 256"
            prev, seen = "", False
            for addr, text in ins[i:]:  # in address order (a small exit block may lie on the way)
                if addr >= syms[name][0] + syms[name][2]:
                    break
                if text.startswith("global_load"):
                    seen = True
                    break
                if text.startswith("s_waitcnt") and "lgkmcnt" in text and not prev.startswith("s_memrealtime"):
                    bad.append(f"{name}: '{text}' between the entry and the first global_load (after '{prev}')")
                    break
                prev = text
            else:
                seen = True  # (unreachable: the loop ends by a break)
            if not seen and not (bad and bad[-1].startswith(name)):
                bad.append(f"{name}: no global_load in the kernel")
    assert not bad, f"{len(bad)} kernels:\n" + "\n".join(bad)
    for k, n in found.items():
        assert n >= MIN_COUNT[k], f"{k}: {n} kernels in the library, expected at least {MIN_COUNT[k]}"

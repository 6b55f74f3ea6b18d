"""Identify the gfx950 code object a kernel was built into (no GPU, no ROCm tools needed).

hipcc embeds one clang offload bundle per translation unit in liblzq.so's .hip_fatbin section:
"__CLANG_OFFLOAD_BUNDLE__", u64 entry count, then per entry u64 offset, u64 size, u64 triple
length and the triple (offsets from the bundle start); the amdgcn entry is the TU's device ELF.
bench.py and tools/summarize_profile.py hash the device ELF that defines the headline kernel, so
a roofline measured by PMC on one build is never reported against another.
"""
from __future__ import annotations

import hashlib
import struct

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def device_objects(lib_path: str, arch: str = "gfx950") -> list[bytes]:
    """The amdgcn code objects for `arch` in the library's offload bundles."""
    with open(lib_path, "rb") as f:
        data = f.read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tlen].decode("ascii", "replace")
            q += 24 + tlen
            if triple.startswith("hip") and "amdgcn" in triple and triple.endswith(arch):
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, q)
    return out


def kernel_object_sha256(lib_path: str, kernel: str = "yields_grid_kernel", arch: str = "gfx950") -> str | None:
    """sha256 of the device code object that defines `kernel` (a substring of its mangled
    name), or None if no code object does."""
    for obj in device_objects(lib_path, arch):
        if kernel.encode() in obj:
            return hashlib.sha256(obj).hexdigest()
    return None


# The sections of a device ELF that make up what the GPU executes: the kernels' machine code
# (.text), their kernel descriptors (.rodata: VGPR/SGPR/LDS/scratch settings) and the code
# object metadata note (.note: arguments, launch bounds).  The whole-object hash above also
# covers the symbol and string tables, which carry clang's per-compilation `__hip_cuid_<hash>`
# symbol -- a hash of the build COMMAND (input paths, flags, output), not of the code: building
# the same source with another command line (e.g. one hipcc per translation unit) changes it.
CODE_SECTIONS = (".note", ".rodata", ".text")


def elf_sections(obj: bytes) -> dict[str, bytes]:
    """Section name -> contents of a little-endian ELF64 object (NOBITS sections are empty)."""
    if obj[:4] != b"\x7fELF" or obj[4] != 2:
        raise ValueError("not an ELF64 object")
    (shoff,) = struct.unpack_from("<Q", obj, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", obj, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", obj, shoff + i * shentsize) for i in range(shnum)]
    str_off = hdrs[shstrndx][4]
    out = {}
    for name_off, typ, _flags, _addr, off, size, *_ in hdrs:
        end = obj.index(b"\0", str_off + name_off)
        name = obj[str_off + name_off:end].decode("ascii", "replace")
        out[name] = b"" if typ == 8 else obj[off:off + size]   # SHT_NOBITS
    return out


def kernel_code_sha256(lib_path: str, kernel: str = "yields_grid_kernel", arch: str = "gfx950") -> str | None:
    """sha256 over CODE_SECTIONS of the device code object that defines `kernel`: equal for two
    builds whose kernels execute the same machine code with the same descriptors, whatever the
    build command (the identity a PMC profile is tied to); None if no code object defines it."""
    for obj in device_objects(lib_path, arch):
        if kernel.encode() in obj:
            secs = elf_sections(obj)
            h = hashlib.sha256()
            for name in CODE_SECTIONS:
                data = secs.get(name, b"")
                h.update(name.encode() + b"\0" + struct.pack("<Q", len(data)) + data)
            return h.hexdigest()
    return None


def elf_symbols(obj: bytes) -> list[tuple[str, int, int, int]]:
    """(name, value, size, section index) of every .symtab entry of a little-endian ELF64 object."""
    (shoff,) = struct.unpack_from("<Q", obj, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", obj, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", obj, shoff + i * shentsize) for i in range(shnum)]
    str_off = hdrs[shstrndx][4]

    def sec_name(h):
        end = obj.index(b"\0", str_off + h[0])
        return obj[str_off + h[0]:end].decode("ascii", "replace")
    names = [sec_name(h) for h in hdrs]
    if ".symtab" not in names:
        return []
    sym = hdrs[names.index(".symtab")]
    strtab = hdrs[sym[6]]  # sh_link: the symbol names' string table
    out = []
    for k in range(sym[5] // 24):
        st_name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", obj, sym[4] + 24 * k)
        end = obj.index(b"\0", strtab[4] + st_name)
        out.append((obj[strtab[4] + st_name:end].decode("ascii", "replace"), value, size, shndx))
    return out


OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def _section_headers(obj: bytes) -> list[tuple]:
    (shoff,) = struct.unpack_from("<Q", obj, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", obj, 0x3A)
    return [struct.unpack_from("<IIQQQQIIQQ", obj, shoff + i * shentsize) for i in range(shnum)]


def _section_names(obj: bytes) -> list[str]:
    """The name of every section, by section index."""
    hdrs = _section_headers(obj)
    str_off = hdrs[struct.unpack_from("<H", obj, 0x3E)[0]][4]
    return [obj[str_off + h[0]:obj.index(b"\0", str_off + h[0])].decode("ascii", "replace") for h in hdrs]


def symbol_bytes(obj: bytes) -> dict[str, bytes]:
    """Symbol name -> the bytes it covers, for every sized .symtab entry that lies in a section with
    contents: the 64-byte kernel descriptors (`*.kd`), the constant tables, the functions."""
    hdrs = _section_headers(obj)
    out = {}
    for name, value, size, shndx in elf_symbols(obj):
        if size and 0 < shndx < len(hdrs) and hdrs[shndx][1] != 8:   # not SHT_NOBITS
            sec = hdrs[shndx]
            out[name] = obj[sec[4] + (value - sec[3]):sec[4] + (value - sec[3]) + size]
    return out


def _masked_descriptor(kd: bytes) -> bytes:
    kd = bytearray(kd)
    kd[16:24] = bytes(8)  # kernel_code_entry_byte_offset: where the code sits, not what it is
    return bytes(kd)


def masked_disassembly(obj: bytes) -> dict[str, list[str]] | None:
    """Function name -> its disassembly, one instruction per entry, with what depends on where the
    code object lays things out masked: the literal of each s_add_u32 / s_addc_u32 that forms a
    PC-relative address after s_getpc_b64.  None if llvm-objdump (ROCm's) is absent or fails."""
    import os
    import re
    import subprocess
    import tempfile
    if not os.path.exists(OBJDUMP):
        return None
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj)
        f.flush()
        r = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f.name],
                           capture_output=True, text=True)
    if r.returncode:
        return None
    funcs, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        t = line.split("//")[0].strip()
        if t:
            cur.append(t)
    for name, lines in funcs.items():
        pcrel = set()
        out = []
        for t in lines:
            op = t.split()[0]
            args = t[len(op):].replace(" ", "").split(",")
            if op == "s_getpc_b64":
                m = re.match(r"s\[(\d+):(\d+)\]", args[0])
                if m:
                    pcrel = {f"s{m.group(1)}", f"s{m.group(2)}"}
            elif op in ("s_add_u32", "s_addc_u32") and args and args[0] in pcrel and len(args) == 3:
                t = f"{op} {args[0]}, {args[1]}, PCREL"
            elif args and args[0] in pcrel:
                pcrel.discard(args[0])  # the register is redefined: no longer a PC-relative base
            out.append(t)
        funcs[name] = out
    return funcs


def kernel_isa_sha256(lib_path: str, kernel: str = "yields_grid_kernel", arch: str = "gfx950") -> str | None:
    """sha256 of the disassembly of the kernels whose mangled names contain `kernel` (every template
    instantiation, in name order), with what depends on where the code object lays them out masked
    (masked_disassembly), and of their kernel descriptors less the code entry offset.
    The identity of a PMC profile of those kernels that survives changes to the other kernels of the
    same translation unit (kernel_code_sha256 hashes the whole object's .text, and the raw bytes of
    a kernel change with the placement of the data it addresses).  None if the kernel or
    llvm-objdump (ROCm's) is absent."""
    for obj in device_objects(lib_path, arch):
        if kernel.encode() not in obj:
            continue
        funcs = masked_disassembly(obj)
        if funcs is None:
            return None
        funcs = {name: lines for name, lines in funcs.items() if kernel in name}
        if not funcs:
            return None
        h = hashlib.sha256()
        for name in sorted(funcs):
            h.update(name.encode() + b"\0" + "\n".join(funcs[name]).encode() + b"\0")
        # and their kernel descriptors (registers, LDS, scratch), less the code entry offset
        for name, kd in sorted(symbol_bytes(obj).items()):
            if kernel in name and name.endswith(".kd") and len(kd) == 64:
                h.update(name.encode() + b"\0" + _masked_descriptor(kd))
        return h.hexdigest()
    return None


def _object_summary(obj: bytes) -> dict:
    secs, syms, names = elf_sections(obj), symbol_bytes(obj), _section_names(obj)
    rodata = names.index(".rodata") if ".rodata" in names else -1
    kds = {n[:-3]: b for n, b in syms.items() if n.endswith(".kd") and len(b) == 64}
    tables = {(n, len(syms[n]), syms[n]) for n, _v, size, shndx in elf_symbols(obj)
              if shndx == rodata and size and not n.endswith(".kd") and n in syms}
    funcs = masked_disassembly(obj) or {}
    isa = {}
    for k, kd in kds.items():
        if k in funcs:
            isa[k] = hashlib.sha256("\n".join(funcs[k]).encode() + b"\0" + _masked_descriptor(kd)).hexdigest()
    return {"text": secs.get(".text", b""), "note": secs.get(".note", b""), "kds": kds, "tables": tables,
            "isa": isa}


def compare_libraries(lib_a: str, lib_b: str, removed: tuple[str, ...] = (), arch: str = "gfx950") -> dict:
    """Whether two builds run the same machine code, code object by code object.

    The `arch` code objects of the two libraries are paired by the kernels they define (most shared
    names).  Per pair the report says whether .text and .note are byte-equal, whether every kernel
    descriptor (the 64 bytes at each `*.kd`) is equal, whether the constant tables of .rodata are
    equal as a set of (name, size, bytes) -- their placement may differ between builds of the same
    code -- and, per kernel present in both, whether its masked disassembly and descriptor
    (kernel_isa_sha256's masking) are equal; and it names the kernels only one side has.

    report["same"]: no difference other than the placement of .rodata tables and the absence from
    `lib_b` of kernels named in `removed` (substrings of mangled names).  An object that lost such a
    kernel may differ in .text, .note and in the descriptors' code entry offsets; its remaining
    kernels must still compare equal."""
    A = [_object_summary(o) for o in device_objects(lib_a, arch)]
    B = [_object_summary(o) for o in device_objects(lib_b, arch)]
    left = list(range(len(B)))
    objects, same = [], True
    for a in A:
        best = max(left, key=lambda j: len(a["kds"].keys() & B[j]["kds"].keys()), default=None)
        if best is None or not (a["kds"].keys() & B[best]["kds"].keys()):
            objects.append({"kernels": sorted(a["kds"]), "only_in_a": sorted(a["kds"]), "only_in_b": [],
                            "unmatched": True})
            same = False
            continue
        left.remove(best)
        b = B[best]
        both = sorted(a["kds"].keys() & b["kds"].keys())
        only_a, only_b = sorted(a["kds"].keys() - b["kds"].keys()), sorted(b["kds"].keys() - a["kds"].keys())
        o = {
            "kernels": both,
            "text_bytes": (len(a["text"]), len(b["text"])),
            "text_sha256": (hashlib.sha256(a["text"]).hexdigest(), hashlib.sha256(b["text"]).hexdigest()),
            "text_equal": a["text"] == b["text"],
            "note_equal": a["note"] == b["note"],
            "descriptors_differ": [k for k in both if a["kds"][k] != b["kds"][k]],
            "descriptors_differ_beyond_entry_offset":
                [k for k in both if _masked_descriptor(a["kds"][k]) != _masked_descriptor(b["kds"][k])],
            "tables_equal": a["tables"] == b["tables"],
            "tables_differ": sorted({t[0] for t in a["tables"] ^ b["tables"]}),
            "isa_differ": [k for k in both if a["isa"].get(k) != b["isa"].get(k) or k not in a["isa"]],
            "only_in_a": only_a, "only_in_b": only_b,
        }
        lost = bool(only_a) and not only_b and all(any(r in k for r in removed) for k in only_a)
        if only_a or only_b:
            ok = lost and not o["descriptors_differ_beyond_entry_offset"]
        else:
            ok = o["text_equal"] and o["note_equal"] and not o["descriptors_differ"]
        o["same"] = bool(ok and o["tables_equal"] and not o["isa_differ"])
        same = same and o["same"]
        objects.append(o)
    for j in left:
        objects.append({"kernels": sorted(B[j]["kds"]), "only_in_a": [], "only_in_b": sorted(B[j]["kds"]),
                        "unmatched": True})
        same = False
    return {"same": same, "objects": objects}

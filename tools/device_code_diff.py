#!/usr/bin/env python3
"""Whether two builds of libpcgym_hip.so carry the same device code, kernel by kernel.

For a refactor of `PCG_DEV` callees the claim to hold is "no kernel changed": this reads both libraries' code objects
(tools/kernel_inventory.py) and reports the kernel count and whether the names are equal, the sha256 of each code object's
`.text`, and for every kernel whose bytes differ its size, every metadata field of the inventory, and whether the two
disassemblies (ROCm llvm-objdump, mnemonics and operands only) are the same multiset of instructions and at how many positions
they differ.

    python tools/device_code_diff.py OLD.so NEW.so

Exit status 0 when every kernel's bytes are equal, 1 otherwise.
"""
import collections
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_inventory as KI  # noqa: E402

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
META = ("vgpr", "agpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch", "dyn_stack", "lds", "max_wg")


def _shdrs(obj):
    """name -> (address, offset, size) of a 64-bit little-endian ELF's sections, and the list in index order"""
    shoff, = struct.unpack_from("<Q", obj, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", obj, 0x3A)
    hdr = [struct.unpack_from("<IIQQQQ", obj, shoff + i * shentsize)[3:6] for i in range(shnum)]
    return {s[0]: h for s, h in zip(KI._sections(obj), hdr)}, hdr


def functions(obj):
    """name -> bytes of every function symbol that lies in a section of the code object"""
    by_name, hdr = _shdrs(obj)
    _, symoff, symsize = by_name[".symtab"]
    _, stroff, _ = by_name[".strtab"]
    out = {}
    for p in range(symoff, symoff + symsize, 24):
        name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", obj, p)
        if info & 0xF != 2 or not 0 < shndx < len(hdr) or not size:  # STT_FUNC, defined
            continue
        addr, off, _ = hdr[shndx]
        end = obj.index(b"\0", stroff + name)
        out[obj[stroff + name:end].decode()] = obj[off + value - addr:off + value - addr + size]
    return out


def text_sha(obj):
    _, off, size = _shdrs(obj)[0][".text"]
    return hashlib.sha256(obj[off:off + size]).hexdigest()


def disassembly(obj, names):
    """name -> the instructions of each named function, a list of 'mnemonic operands' strings"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj)
        f.flush()
        txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", "--disassemble-symbols=" + ",".join(names), f.name],
                             capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in names else cur  # (a label inside a function is not in `names`)
            continue
        line = line.split("//")[0].strip()
        if cur is not None and line:
            cur.append(" ".join(line.split()))
    return out


class Lib:
    def __init__(self, path):
        self.objs = KI.device_objects(path)
        self.inv = {k["name"]: k for k in KI.inventory(path)}
        self.code, self.where = {}, {}
        for i, obj in enumerate(self.objs):
            for name, b in functions(obj).items():
                if name in self.inv and name not in self.code:  # (the first unit's copy, as the inventory keeps)
                    self.code[name], self.where[name] = b, i


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = Lib(sys.argv[1]), Lib(sys.argv[2])
    print(f"kernels: {len(old.inv)} / {len(new.inv)}, names {'equal' if old.inv.keys() == new.inv.keys() else 'DIFFER'}")
    for n in sorted(old.inv.keys() ^ new.inv.keys()):
        print(f"  only in {'old' if n in old.inv else 'new'}: {n}")
    print(f"code objects: {len(old.objs)} / {len(new.objs)}; sha256 of .text, old and new")
    for i in range(max(len(old.objs), len(new.objs))):
        so = text_sha(old.objs[i]) if i < len(old.objs) else "-"
        sn = text_sha(new.objs[i]) if i < len(new.objs) else "-"
        print(f"  [{i}] {so} {sn} {'same' if so == sn else 'DIFFERENT'}")
    common = sorted(old.inv.keys() & new.inv.keys())
    diff = [n for n in common if old.code[n] != new.code[n]]
    fams = collections.Counter(old.inv[n]["family"] for n in diff)
    print(f"kernels with equal bytes: {len(common) - len(diff)} of {len(common)}; differing: {len(diff)}"
          + "".join(f"\n  {f}: {c}" for f, c in sorted(fams.items())))
    dis = {}
    for lib in (old, new):
        per_obj = collections.defaultdict(list)
        for n in diff:
            per_obj[lib.where[n]].append(n)
        for i, names in per_obj.items():
            dis.update({(id(lib), n): v for n, v in disassembly(lib.objs[i], names).items()})
    for n in diff:
        a, b = dis[(id(old), n)], dis[(id(new), n)]
        ko, kn = old.inv[n], new.inv[n]
        meta = " ".join(f"{m}={ko[m]}" if ko[m] == kn[m] else f"{m}={ko[m]}->{kn[m]}" for m in META)
        multiset = collections.Counter(a) == collections.Counter(b)
        pos = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
        print(f"{ko['demangled']}\n  bytes {len(old.code[n])} -> {len(new.code[n])}; {meta}\n"
              f"  instructions {len(a)} -> {len(b)}; multiset {'same' if multiset else 'DIFFERENT'}; positions that differ: {pos}")
    return 1 if diff or old.inv.keys() != new.inv.keys() else 0


if __name__ == "__main__":
    sys.exit(main())

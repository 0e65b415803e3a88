"""Compare the device code of two builds kernel by kernel: python tools/compare_code_objects.py A.elf B.elf

A.elf / B.elf: gfx950 code objects, e.g. of a device-only compile with the product flags
    hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC -I include --cuda-device-only -c gaussianvi_amd/csrc/gvi_hip.hip -o X.co
    clang-offload-bundler --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 --input=X.co --output=X.elf --unbundle
Prints whether the two have the same symbols, and every function whose code bytes or whose kernel descriptor (registers, LDS,
scratch, kernarg size -- everything but the code-entry offset, which moves with the function) differ.  A host-only change
may permute the functions (another instantiation order) and changes the __hip_cuid_* symbol; it changes nothing else.
Exit status 1 if anything else differs."""
import struct
import sys


def load(path):
    b = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, _, addr, off, size, link, _, _, _ = struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize)
        secs.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link))

    def cstr(tab, o):
        return b[tab["off"] + o:b.index(b"\0", tab["off"] + o)].decode()
    for s in secs:
        s["n"] = cstr(secs[shstrndx], s["name"])
    symtab = next(s for s in secs if s["type"] == 2)
    out = {}
    for i in range(symtab["size"] // 24):
        nm, info, _, shndx, val, size = struct.unpack_from("<IBBHQQ", b, symtab["off"] + i * 24)
        if shndx == 0 or shndx >= len(secs) or size == 0:
            continue
        sec = secs[shndx]
        start = sec["off"] + val - sec["addr"]
        out[cstr(secs[symtab["link"]], nm)] = (info & 15, b[start:start + size])
    return out


def main():
    A, B = load(sys.argv[1]), load(sys.argv[2])
    bad = 0
    for k in sorted(set(A) ^ set(B)):
        print("only in one:", k)
        bad += not k.startswith("__hip_cuid_")
    nf = nk = 0
    for k in sorted(set(A) & set(B)):
        (ta, da), (_, db) = A[k], B[k]
        if k.endswith(".kd"):
            nk += 1
            same = da[:16] + da[24:] == db[:16] + db[24:]
        else:
            nf += ta == 2
            same = da == db
        if not same:
            print("differs:", k)
            bad += 1
    print(f"{nf} functions and {nk} kernel descriptors compared, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

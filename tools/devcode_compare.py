#!/usr/bin/env python3
"""Are two builds' gfx950 code objects the same device code?  For a host-only change the answer must be yes.

    hipcc <the Makefile's FLAGS> -I include --cuda-device-only --no-gpu-bundle-output -c -o A.co gqhip.hip    (in each tree)
    python tools/devcode_compare.py [--all] A.co B.co [A2.co B2.co ...]      # --all: every differing name, not the first five

Compares, per pair: the set of function symbols (llvm-readelf -sW), every function's disassembly (llvm-objdump -d without
addresses; a pc-relative reference -- s_getpc_b64 + s_add_u32 -- is compared as the symbol + offset it resolves to, so emission
order may differ and nothing else), the bytes of every data object (constant tables whole; kernel descriptors except their
entry offset, which is a position) and every kernel's metadata record (llvm-readelf --notes: registers, LDS, scratch,
arguments).  Needs no GPU.  Exit status 1 on any difference."""
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def symbols(path):
    """[(name, type, address, size, section index)] of the defined symbols, once per name"""
    seen, out = set(), []
    for line in run(LLVM + "llvm-readelf", "-sW", path).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND" and f[7] not in seen:
            seen.add(f[7])
            out.append((f[7], f[3], int(f[1], 16), int(f[2]), f[6]))
    return out


def functions(path):
    return {s[0] for s in symbols(path) if s[1] == "FUNC"}


def objects(path):
    """{name: bytes} of the data objects; a kernel descriptor (.kd) without its kernel_code_entry_byte_offset (bytes 16..23)"""
    syms = [s for s in symbols(path) if s[1] == "OBJECT" and s[3] > 0]
    out = {}
    for index in {s[4] for s in syms}:
        sec = [m for m in (re.match(rf"\s*\[\s*{index}\]\s+(\S+)\s+(\S+)\s+([0-9a-f]+)", l)
                           for l in run(LLVM + "llvm-readelf", "-SW", path).splitlines()) if m][0]
        name, kind, addr = sec.group(1), sec.group(2), int(sec.group(3), 16)
        if kind == "NOBITS":
            continue
        data = bytearray()
        for l in run(LLVM + "llvm-readelf", "-x", name, path).splitlines():
            m = re.match(r"^0x[0-9a-f]+ ((?:[0-9a-f]{2,8} ?){1,4})", l)
            if m:
                data += bytes.fromhex(m.group(1).replace(" ", ""))
        for s in syms:
            if s[4] == index:
                b = bytes(data[s[2] - addr:s[2] - addr + s[3]])
                out[s[0]] = b[:16] + b[24:] if s[0].endswith(".kd") else b
    return out


def disassembly(path):
    """{symbol: [instruction text]} -- position-independent: no addresses, no encodings; the literal of the s_add_u32 after an
    s_getpc_b64 (a pc-relative reference) is replaced by the symbol + offset it points at"""
    syms = sorted((s[2], s[2] + max(s[3], 1), s[0]) for s in symbols(path))
    body, cur, getpc = {}, None, False
    for line in run(LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", path).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = body.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if cur is None or not m:
            continue
        text, addr = m.group(1), int(m.group(2), 16)
        lit = re.match(r"^(s_add_u32 \S+ \S+) (0x[0-9a-f]+|-?\d+)$", text)
        if getpc and lit:
            v = int(lit.group(2), 0) & 0xFFFFFFFF
            target = addr + (v - (1 << 32) if v >> 31 else v)      # s_getpc_b64 returned the address of this instruction
            hit = [(lo, n) for lo, hi, n in syms if lo <= target < hi]
            text = f"{lit.group(1)} <{hit[0][1]}+{target - hit[0][0]}>" if hit else f"{lit.group(1)} <unresolved {target:#x}>"
        getpc = text.startswith("s_getpc_b64")
        cur.append(text)
    return body


def metadata(path):
    """{kernel symbol: its amdhsa.kernels record as text}"""
    notes = run(LLVM + "llvm-readelf", "--notes", path)
    recs = {}
    for chunk in re.split(r"\n(?=\s*- \.agpr_count:|\s*- \.args:)", notes):
        m = re.search(r"\.symbol:\s+'?([^\s']+)", chunk)
        if m:
            recs[m.group(1)] = chunk.split("amdhsa.target")[0].strip()
    return recs


def compare(a, b, shown=5):
    fa, fb = functions(a), functions(b)
    da, db = disassembly(a), disassembly(b)
    oa, ob = objects(a), objects(b)
    ma, mb = metadata(a), metadata(b)
    diff_code = sorted(s for s in fa & fb if da.get(s) != db.get(s))
    diff_obj = sorted(s for s in set(oa) | set(ob) if oa.get(s) != ob.get(s))
    diff_meta = sorted(s for s in set(ma) | set(mb) if ma.get(s) != mb.get(s))
    unresolved = sum(t.count("<unresolved") for d in (da, db) for body in d.values() for t in body)
    print(f"{a}\n  vs {b}")
    print(f"  function symbols: {len(fa)} vs {len(fb)}; only in first {sorted(fa - fb)}; only in second {sorted(fb - fa)}")
    print(f"  instructions compared: {sum(len(da.get(s, [])) for s in fa & fb)}; functions whose disassembly differs: {len(diff_code)} {diff_code[:shown]};"
          f" pc-relative references left unresolved: {unresolved}")
    print(f"  data objects (kernel descriptors, constant tables): {len(oa)} vs {len(ob)}; differing: {len(diff_obj)} {diff_obj[:shown]}")
    print(f"  kernel metadata records: {len(ma)} vs {len(mb)}; differing: {len(diff_meta)} {diff_meta[:shown]}")
    same = (fa == fb and not diff_code and not diff_obj and not diff_meta and not unresolved and len(ma) == len(mb) == len(fa) > 0
            and all(da.get(s) for s in fa))
    print("  IDENTICAL device code" if same else "  DIFFERENT")
    return same


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--all"]
    shown = None if "--all" in sys.argv[1:] else 5
    assert args and len(args) % 2 == 0, __doc__
    results = [compare(args[i], args[i + 1], shown) for i in range(0, len(args), 2)]   # (every pair is reported)
    sys.exit(0 if all(results) else 1)

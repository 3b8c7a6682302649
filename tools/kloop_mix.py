"""Instruction mix of the innermost K-tile loop of every gemm_bf16_w4_kernel instantiation in a
device listing (hipcc -S --cuda-device-only of csrc/gemm_bf16_w4.hip with the Makefile's flags):

  python tools/kloop_mix.py LISTING.s [LISTING2.s ...]

The loop is the shortest backward-branch span of a kernel that holds at least 100 MFMAs (one K-tile is
128).  Static counts per K-tile: MFMA, ds_read_b128, LDS-DMA pieces, s_waitcnt, scalar ALU (every s_*
except waits, barriers, nops and branches; the tile-change path of advance() lies inside the span and
is counted although it runs once per tile), VALU (v_* except MFMA), then the kernel's register lines.
"""
import re
import sys

_SKIP = ("s_waitcnt", "s_barrier", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_setprio", "s_sleep")


def functions(path):
    name, body = None, []
    for raw in open(path):
        ln = raw.split(";")[0].strip() if not raw.lstrip().startswith(";;#") else ""
        m = re.match(r"^(_Z\w+):", raw)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if raw.startswith(".Lfunc_end"):
            yield name, body
            name = None
            continue
        if ln:
            body.append(ln)


def resources(path):
    out, name = {}, None
    for raw in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", raw)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.match(r"\s*\.amdhsa_next_free_(vgpr|sgpr) (\d+)", raw)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
        m = re.match(r"\s*\.amdhsa_private_segment_fixed_size (\d+)", raw)
        if m and name:
            out[name]["scratch"] = int(m.group(1))
        m = re.match(r"\s*\.amdhsa_accum_offset (\d+)", raw)
        if m and name:
            out[name]["accum_offset"] = int(m.group(1))
    return out


def kloop(body):
    labels = {ln[:-1]: i for i, ln in enumerate(body) if ln.endswith(":")}
    best = None
    for i, ln in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\S+)", ln)
        if not m or m.group(1) not in labels or labels[m.group(1)] > i:
            continue
        span = body[labels[m.group(1)]:i + 1]
        if sum(s.startswith("v_mfma") for s in span) >= 100 and (best is None or len(span) < len(best)):
            best = span
    return best


def mix(span):
    c = dict(mfma=0, ds_read_b128=0, lds_dma=0, s_waitcnt=0, salu=0, valu=0, m0_writes=0, lgkm_waits=0)
    for s in span:
        mn = s.split()[0]
        if s.endswith(":"):
            continue
        if mn.startswith("v_mfma"):
            c["mfma"] += 1
        elif mn == "ds_read_b128":
            c["ds_read_b128"] += 1
        elif mn.startswith("buffer_load") and s.rstrip().endswith("lds"):
            c["lds_dma"] += 1
        elif mn == "s_waitcnt":
            c["s_waitcnt"] += 1
            c["lgkm_waits"] += "lgkmcnt" in s
        elif mn.startswith("s_") and not mn.startswith(_SKIP):
            c["salu"] += 1
            c["m0_writes"] += bool(re.match(r"\S+\s+m0\b", s))
        elif mn.startswith("v_"):
            c["valu"] += 1
    return c


def short(name):
    m = re.search(r"gemm_bf16_w4_kernelILi(\d+)ELb(\d)ELb(\d)ELi(\d+)ELb(\d)E", name)
    if not m:
        return None
    e, nopad, s3, abl, avid = m.groups()
    return f"<{e},{'true' if nopad == '1' else 'false'},{'true' if s3 == '1' else 'false'}" + (
        f",{abl},true>" if avid == "1" else ">")


if __name__ == "__main__":
    for path in sys.argv[1:]:
        print(f"== {path}")
        res = resources(path)
        for name, body in functions(path):
            tag = short(name)
            span = kloop(body) if tag else None
            if not span:
                continue
            c = mix(span)
            r = res.get(name, {})
            print(f"{tag:22s} mfma {c['mfma']:3d}  ds_read_b128 {c['ds_read_b128']:2d}  lds-dma {c['lds_dma']:2d}  "
                  f"s_waitcnt {c['s_waitcnt']:2d} (lgkmcnt {c['lgkm_waits']:2d})  salu {c['salu']:3d} (m0 writes "
                  f"{c['m0_writes']:2d})  valu {c['valu']:2d}  | vgpr {r.get('vgpr')} (accum_offset "
                  f"{r.get('accum_offset')}) sgpr {r.get('sgpr')} scratch {r.get('scratch')}")

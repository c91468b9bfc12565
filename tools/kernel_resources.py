"""Resource table of the kernels of one translation unit, from its gfx950 assembly (tools/isa.sh UNIT.hip > unit.s):

    python tools/kernel_resources.py window_f1 parent_window.s new_window.s [parent_batch.s new_batch.s ...]

Files are taken in (before, after) pairs.  Per kernel whose name contains the filter: VGPRs, SGPRs, scratch bytes, waves per
SIMD by registers (512 VGPRs per lane, allocated in steps of 8, at most 8 waves) and the static counts of v_mul_f64,
v_add_f64 and LDS reads.  A line ends in `!` when scratch is not 0 or a fp64 count differs between the two files."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, re.S | re.M):
        body = m.group(0)
        out[m.group(1)] = {k: len(re.findall(r"^\s+" + k + r"\b", body, re.M))
                           for k in ("v_mul_f64", "v_add_f64", "ds_read_b128", "ds_read_b64")}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.S | re.M):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if name in out:
            for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size"):
                out[name][k] = int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
    return out


def demangle(names):
    """window_f1_kernel<4, 8, true, false> from _ZN3sdp16window_f1_kernelILi4ELi8ELb1ELb0EEEv... (integer and bool arguments)"""
    out = {}
    for n in names:
        m = re.match(r"_ZN3sdp\d+(\w+?)I((?:L[ib]\d+E)+)E", n)
        args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", m.group(2))]
        out[n] = f"{m.group(1)}<{', '.join(args)}>"
    return out


def waves(vgpr):
    return min(8, 512 // (-(-vgpr // 8) * 8))


def main():
    flt, files = sys.argv[1], sys.argv[2:]
    print(f"{'kernel':44s} {'VGPR':>9s} {'waves':>6s} {'SGPR':>8s} {'scratch':>7s} {'v_mul_f64':>10s} {'v_add_f64':>10s} "
          f"{'ds_read_b128':>12s} {'ds_read_b64':>11s}   (before -> after)")
    for before, after in zip(files[0::2], files[1::2]):
        a, b = kernels(before), kernels(after)
        names = demangle(sorted(n for n in b if flt in n))
        # (paired by the demangled name: a kernel whose parameter list changed has another mangled one)
        old = {v: k for k, v in demangle(sorted(n for n in a if flt in n)).items()}
        for n in sorted(names, key=names.get):
            # (a template parameter added at the end, with a default: the kernel without its last argument is the counterpart)
            was = names[n] if names[n] in old else names[n].rsplit(", ", 1)[0] + ">"
            x, y = a[old[was]], b[n]
            bad = y["private_segment_fixed_size"] or x["private_segment_fixed_size"] or any(x[k] != y[k] for k in ("v_mul_f64", "v_add_f64"))
            pair = lambda k: f"{x[k]}->{y[k]}"
            print(f"{names[n]:44s} {pair('vgpr_count'):>9s} {waves(x['vgpr_count'])}->{waves(y['vgpr_count']):<3d} {pair('sgpr_count'):>8s} "
                  f"{pair('private_segment_fixed_size'):>7s} {pair('v_mul_f64'):>10s} {pair('v_add_f64'):>10s} {pair('ds_read_b128'):>12s} "
                  f"{pair('ds_read_b64'):>11s}{' !' if bad else ''}")


if __name__ == "__main__":
    main()

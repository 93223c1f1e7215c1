"""Compares two builds kernel by kernel and field by field: python tools/compare_kernel_usage.py OLD.log NEW.log, the logs being the output of
`python renderer-rs_amd/build.py --force --usage` (-Rpass-analysis=kernel-resource-usage) of the two trees.  Prints the kernels whose VGPR, SGPR,
spill, scratch, LDS or occupancy figures moved and the figures of the kernels only the new build has; exit status 1 if an existing kernel moved."""
import re
import sys


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][A-Za-z0-9 \[\]/-]+): (\S+)", line)
        if m and cur is not None:
            cur.setdefault(m.group(1).strip(), m.group(2))
    return out


def main():
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    moved = [k for k in old if old[k] != new.get(k)]
    print(f"{len(old)} kernels in the old build, {len(new)} in the new one; existing kernels whose figures moved: {moved or 'none'}")
    for k in moved:
        print(" ", k, old[k], "->", new.get(k))
    for k in new:
        if k not in old:
            print("new:", k, new[k])
    sys.exit(1 if moved else 0)


if __name__ == "__main__":
    main()

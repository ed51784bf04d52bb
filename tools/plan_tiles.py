"""Which tile every conv of a pass runs with, and how many pixels its grid computes for the pixels the map has.

    MI355_SCHED_LOG=1 python bench.py ... 2> run.log ; python tools/plan_tiles.py run.log

Reads the engine's "[tile]" lines (one per launched conv of the shape planned last) and prints, for the LDS-staged kernels
(version 1), the block's pixels P = WP * PT * 16, the tiles per image and the padding: tiles * P against Wout * Hout.  The
candidates a shape COULD run with come from ops.plan_tiles() (host-only)."""
import re
import sys

pat = re.compile(r"\[tile\] (\S+) v(\d+) PT(\d+) CT(\d+) WP(\d+) tile (\d+)x(\d+) G(\d+) grid (\d+)x(\d+) map (\d+)x(\d+) x(\d+)( \+1x1)?")
rows = {}
for line in open(sys.argv[1]):
    m = pat.search(line)
    if m:
        rows[m.group(1)] = m          # a shape planned twice (warm-up, then the run): the last one counts
print(f"{'conv':42s} {'kernel':>4s} {'PT':>2s} {'CT':>2s} {'WP':>2s} {'tile':>7s} {'map':>9s} {'blocks/img':>10s} {'pixels computed':>15s} {'of map':>7s}")
tot_c = tot_m = 0
for name, m in rows.items():
    v, pt, ct, wp, tw, th, g, gx, gy, w, h, nimg = (int(x) for x in m.groups()[1:13])
    if v != 1 or h == 1:                # streaming / pipelined / split-K kernels and flattened pointwise maps: no 2-D tile
        continue
    P = wp * pt * 16
    tiles = -(-w // tw) * -(-h // th)
    tot_c += tiles * P; tot_m += w * h
    print(f"{name[:40] + (m.group(14) or ''):42s} {'v1':>4s} {pt:2d} {ct:2d} {wp:2d} {tw:3d}x{th:<3d} {w:4d}x{h:<4d} {tiles:10d} {tiles * P:15d} {tiles * P / (w * h):7.3f}")
if tot_m:
    print(f"all 3x3 launches: {tot_c} pixels computed for {tot_m} ({tot_c / tot_m:.3f})")

"""The column-block plans of the tuned 16-bit kernels, restated once in Python (test infrastructure, no GPU, no library).

Wide rows are cut into one to four column blocks by two host functions:
  - rn_stage23_plan (csrc/rn_stage23x.hip): the fused stage pair 2+3.  As few blocks as fit the widest ring row, of equal width +-1;
    a block reads its output columns + 10 input columns, which must lie in X_WMIN .. X_WMAX.
  - rn_colblock_plan (csrc/rn_stage.h): stages 4, 5 and 6 (rn_stage4x/5x/6x.hip).  The fewest blocks of equal width +-1 whose widths
    lie in the kernel's [wo_min, wo_max] output columns.
A plan is a list of (first output column, output columns) per block, or None where the kernel does not take the shape (another
kernel runs).  tests/test_seam_cases_host.py pins the plans of the seam sides."""

X_WMIN, X_WMAX = 193, 215             # rn_stage23x.hip: input columns of a block of the pair
# family -> (wo_min, wo_max): output columns per block
#   stage 4 (rn_stage4x.hip, U_WMIN = 193, U_WMAX = 206): 2 wo + 4 input columns in U_WMIN + 1 .. U_WMAX
#   stage 5 (rn_stage5x.hip, V_WMIN = 66, V_WMAX = 110):  2 wo + 4 .. 2 wo + 6 staged input columns in V_WMIN .. V_WMAX
#   stage 6 (rn_stage6x.hip, S6_WMIN = 35, S6_WMAX = 50): wo + 2 input columns
WIDTH_LIMITS = {4: ((193 + 1 - 4 + 1) // 2, (206 - 4) // 2), 5: ((66 - 4 + 1) // 2, (110 - 4) // 2), 6: (35 - 2, 50 - 2)}
MIN_IN_SIDE = {4: 193, 5: 66, 6: 35}
FAMILIES = ("pair", 4, 5, 6)


def colblock_plan(out_side, wo_min, wo_max):
    """rn_colblock_plan: [(xo0, wo)] of the fewest blocks (<= 4) of equal width +-1 with widths in [wo_min, wo_max], or None."""
    for nb in range(1, 5):
        hi, lo = (out_side + nb - 1) // nb, out_side // nb
        if hi > wo_max or lo < wo_min:
            continue
        widths = [lo + (1 if b < out_side % nb else 0) for b in range(nb)]
        return [(sum(widths[:b]), widths[b]) for b in range(nb)]
    return None


def stage23_plan(in_side):
    """rn_stage23_plan: [(x0, wo)] of the pair's blocks over its in_side - 10 output columns, or None."""
    out = in_side - 10
    if out < X_WMIN - 10:
        return None
    nb = (out + (X_WMAX - 10) - 1) // (X_WMAX - 10)
    if nb > 4:
        return None
    base, rem = out // nb, out % nb
    if base + 10 < X_WMIN:
        return None
    widths = [base + (1 if b < rem else 0) for b in range(nb)]
    return [(sum(widths[:b]), widths[b]) for b in range(nb)]


def stage_plan(graph, k):
    """The plan of the row-blocked kernel of stage 4, 5 or 6 of ``graph`` (rn_stage4x/5x/6x_supported), or None."""
    s = graph.stages[k]
    if s.in_side < MIN_IN_SIDE[k]:
        return None
    if k == 5 and (s.skip_side != s.in_side or s.in_side - 2 * s.out_side > 5):
        return None
    return colblock_plan(s.out_side, *WIDTH_LIMITS[k])


def block_plans(graph):
    """family ("pair", 4, 5, 6) -> [(first output column, output columns)] per block, or None."""
    out = {"pair": stage23_plan(graph.stages[2].in_side)}
    for k in (4, 5, 6):
        out[k] = stage_plan(graph, k)
    return out


def block_counts(graph):
    """family -> number of blocks (0: the kernel does not take this side)."""
    return {f: len(p) if p else 0 for f, p in block_plans(graph).items()}


def seam_columns(graph):
    """Stage that owns the seams (3 for the pair: its output is what the pair stores) -> first output column of every block but the first."""
    plans = block_plans(graph)
    return {(3 if f == "pair" else f): [x0 for x0, _ in p[1:]] for f, p in plans.items() if p}

"""Shared inputs of test_cells_cpu.py / test_cells_gpu.py: THE RULE of include/mmft_cells.h as a literal triple loop (cell, pin,
row) that also says why a cell is not selected, and synthetic cell sets over an incidence of their own whose first cells are
made to show every edge of the rule.  A plain module: it holds no test."""
import numpy as np

from mmft import cells as CL

I64 = lambda v: np.asarray(v, dtype=np.int64)
NODE_OFF = 3                              # the design's nodes start behind three of another design
SIZES = (0, 1, 8, 64, 65)
SPANS = (1, 31, 32, 33, 64, 65, 2049)     # the bitmap's word edges
COUNTS = (1, 2, 4, 5, 63, 257)            # cells: one wave, part of a workgroup, one, more than one, many
LONG = 300                                # rows of the long pin: more than four rounds of a wave
# the slack of row row_lo + b by b % 8: below, above, NaN, exactly 0, -0.0 before the rule's + 0.0f, exactly -0.25, below, above
KINDS = ('below', 'above', 'nan', 'zero', 'minus_zero', 'quarter', 'below', 'above')


def make(C, span, row_lo=5, seed=0):
    """C cells over rows [row_lo, row_lo + span) of T = row_lo + span + LONG + 7.  The first cells are crafted (as far as C and the span
    allow), the others seeded.  dict(inc=(ptr, rows) int64 over NODE_OFF + n nodes, pins (the design's own ids), cell_ptr, pred,
    required, row_lo, span, T, tags: {name: cell})."""
    rng = np.random.default_rng(1000 * seed + 7 * C + span)
    T = row_lo + span + LONG + 7
    b = np.arange(T) - row_lo
    kind = np.array([KINDS[v % 8] for v in b])
    required = rng.uniform(1.0, 2.0, T).astype(np.float32)
    slack = np.where(np.isin(kind, ['below']), -rng.uniform(0.5, 3.0, T), rng.uniform(0.5, 3.0, T)).astype(np.float32)
    pred = (required - slack).astype(np.float32)
    pred[kind == 'nan'] = np.nan
    for name, req, prd in (('zero', 0.75, 0.75), ('minus_zero', -0.0, 0.0), ('quarter', 1.0, 1.25)):
        required[kind == name], pred[kind == name] = req, prd
    inside = np.arange(row_lo, row_lo + span)
    of_kind = lambda name: inside[kind[inside] == name]
    some = lambda name: (of_kind(name)[:1] if of_kind(name).size else inside[:1])       # (a span too short for the kind: any row)

    def random_rows(most=6):
        return np.sort(rng.choice(inside, min(int(rng.integers(0, most + 1)), span), replace=False))

    twin = np.sort(rng.choice(inside, min(span, 3), replace=False))
    long_pool = np.arange(T) if span < 2 * LONG else inside
    shared = inside[:min(span, 5)]
    crafted = [
        ('long', [np.sort(rng.choice(long_pool, min(LONG, long_pool.size), replace=False)), twin, twin.copy(),
                  np.array([row_lo - 1, row_lo]), np.array([row_lo + span - 1, row_lo + span]), random_rows(), random_rows(), random_rows()]),
        ('ends', [np.unique([row_lo, row_lo + span - 1])]),
        ('sixty_four', [random_rows(4) for _ in range(64)]),
        ('no_pins', []),
        ('sixty_five', [random_rows(2) for _ in range(65)]),
        ('no_rows', [np.zeros(0, dtype=np.int64)]),
        ('nan_only', [some('nan')]),
        ('zero', [some('zero')]),
        ('minus_zero', [some('minus_zero')]),
        ('quarter', [some('quarter')]),
        ('sharing', [shared, shared[::2], shared[1:], random_rows(), random_rows(), random_rows(), random_rows(), random_rows()]),
        ('outside_only', [np.array([row_lo - 1]), np.array([row_lo + span])]),
    ]
    lists, sizes, tags = [], [], {}
    for c in range(C):
        if c < len(crafted):
            tags[crafted[c][0]] = c
            mine = crafted[c][1]
        else:
            mine = [random_rows() for _ in range(int(rng.choice(SIZES)))]
        lists += [I64(v) for v in mine]
        sizes.append(len(mine))
    M = len(lists)
    n = M + 2                                                   # two pins of no cell
    where = rng.permutation(n)[:M]                              # the node of each pin: the design's own numbering
    per_node = [I64([])] * (NODE_OFF + n)
    for m, v in enumerate(lists):
        per_node[NODE_OFF + where[m]] = v
    per_node[0] = I64(inside[:2])                               # (the other design's nodes lie on rows too)
    ptr = I64(np.concatenate([[0], np.cumsum([len(v) for v in per_node])]))
    rows = I64(np.concatenate(per_node)) if ptr[-1] else I64([])
    return dict(inc=(ptr, rows), pins=I64(where), cell_ptr=I64(np.concatenate([[0], np.cumsum(sizes)])), pred=pred, required=required,
                row_lo=row_lo, span=span, T=T, tags=tags, C=C)


def literal(case, thr):
    """Per cell, by a literal triple loop: dict(sel, worst (np.float32 or None), rows (sorted list), why (None where selected),
    visits (pairs inside the range), outside (pairs outside it), below (violating pairs), longest (rows of its longest pin))."""
    ptr, rows = case['inc']
    pred, required, lo, span = case['pred'], case['required'], case['row_lo'], case['span']
    out = []
    for c in range(case['C']):
        pins = case['pins'][case['cell_ptr'][c]:case['cell_ptr'][c + 1]]
        seen, worst, below, visits, outside, longest = set(), None, 0, 0, 0, 0
        if 1 <= len(pins) <= 64:
            for n in pins:
                g = int(n) + NODE_OFF
                longest = max(longest, int(ptr[g + 1] - ptr[g]))
                for r in rows[ptr[g]:ptr[g + 1]]:
                    r = int(r)
                    if not lo <= r < lo + span:
                        outside += 1
                        continue
                    visits += 1
                    seen.add(r)
                    with np.errstate(invalid='ignore'):
                        s = (np.float32(required[r]) - np.float32(pred[r])) + np.float32(0.0)
                    if s != s:
                        continue
                    if worst is None or s < worst:
                        worst = s
                    if thr is not None and s < np.float32(thr):
                        below += 1
        if len(pins) == 0:
            why = 'no_pins'
        elif len(pins) > 64:
            why = 'many_pins'
        elif thr is None:
            why = None
        elif not seen:
            why = 'no_rows'
        elif worst is None:
            why = 'nan_only'
        elif below == 0:
            why = 'not_below'
        else:
            why = None
        out.append(dict(sel=why is None, worst=worst, rows=sorted(seen), why=why, visits=visits, outside=outside, below=below, longest=longest))
    return out


def host(case, thr):
    """(sel, n_rows, n_pins, worst) of cells.count_host on a case."""
    return CL.count_host(case['inc'], NODE_OFF, case['pins'], case['cell_ptr'], case['pred'], case['required'], case['row_lo'], case['span'], thr)


def expected(case, thr):
    """(cells, tables, words) a device build of a case must equal: cells.critical_host -> search.plan_tables -> the layout;
    words None where nothing is selected."""
    chosen, worst = CL.critical_host(case['inc'], NODE_OFF, case['pins'], case['cell_ptr'], case['pred'], case['required'], case['row_lo'],
                                     case['span'], thr)
    if chosen.size == 0:
        return chosen, None, None
    tables = CL.plan_host(case['inc'], NODE_OFF, case['pins'], case['cell_ptr'], chosen, case['row_lo'], case['span'])
    return chosen, tables, CL.words(tables, chosen, worst)

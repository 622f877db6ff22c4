"""The plan of tests/test_gpu_fused_cells.py: which engine options launch which instantiation of the fused kernel
k_em_fused<P, MODE, FMT, GEO, PROF, IX> — one leg per layout, every leg with the exact set of cells (the six template values, as
the launch census of `_lib.Engine.fused_launches` names them) it must launch unconditionally.  tests/test_fused_cells_host.py holds
the plan to the committed list of kernels without a GPU: a kernel that is added to the table (fz_exists, tsem_fused.h) has no leg
until a line below names it, and that file fails until then.

How the options reach a cell (tsem_setup.hip: tsem_choose_geometry, layout_decide_format; tsem_em.hip: em_pass_impl, launch_lnl,
launch_fused):
  P      option `parts`;  GEO  option `geometry` (0, 2, 3 for teams of 1-4; 1, 2 for teams of 5-8);
  FMT    1: `value_format` 2 (score codes); 2: `value_format` 1 (fp64 entries, score table in LDS); 0: `value_format` 1 with a score
         table of 3000 entries (too long for LDS: fp64 row weights);
  IX     fp64 entries of a non-split layout: `index_format` 1 (3 bytes) or 2 (the quad index; geometry 0 or 1); 0 (32 bits) elsewhere;
  MODE   0 em_pass; 1 / 9 lnl_pass with `fused_dbg` 8192 / 32768 (unforced, and with 16384 alone, the launch is armed with the device's
         choice between the two and counts as conditional); 2 / 3 em_pass under `reproducible` 2 / 1; 4 em_chunk with use_likelihood on a
         layout built with `use_likelihood`; 5, 7 em_pass and 5, 8 lnl_pass on the split layout (`split` 1, teams of 5-8);
  PROF   `fused_prof` 1: em_pass launches the timeline kernel."""
import collections
import itertools

KINDS = ('plain', 'repro2', 'repro1', 'lnl4', 'split', 'prof')
# the modes a leg of each kind launches unconditionally, where the kernel exists (MODE 9 needs the score table in LDS: not FMT 0)
MODES = {'plain': (0, 1, 9), 'repro2': (2,), 'repro1': (3,), 'lnl4': (4,), 'split': (5, 7, 8), 'prof': (0,)}
Leg = collections.namedtuple('Leg', 'name kind P geo fmt ix options matrix big_lut forms cells')
FZ_NS = 6                                         # tsem_fused.h: register sets of a data wave
STEADY = FZ_NS + 1                                # blocks every team must walk: every register set refilled, the offs ring, both s slots and
                                                  # every y slot reused, four exchange slots rewritten... past the prologue's five blocks
SMALL, LARGE = (1, 2, 3, 4), (5, 6, 7, 8)

# kind, team sizes, geometries, (FMT, IX) pairs: every line is a family of legs, one per combination
PLAN = (
    ('plain', SMALL, (0,), ((0, 1), (0, 2), (1, 0), (2, 1), (2, 2))),
    ('plain', SMALL, (2, 3), ((0, 1), (1, 0), (2, 1))),
    ('plain', LARGE, (1,), ((0, 1), (0, 2), (1, 0), (2, 1), (2, 2))),
    ('plain', LARGE, (2,), ((0, 1), (1, 0), (2, 1))),
    ('repro2', SMALL, (0, 2, 3), ((1, 0), (2, 1))),
    ('repro2', LARGE, (1, 2), ((1, 0), (2, 1))),
    ('repro1', SMALL, (0, 2, 3), ((1, 0),)),
    ('repro1', LARGE, (1, 2), ((1, 0),)),
    ('lnl4', SMALL, (0, 2), ((1, 0),)),
    ('lnl4', LARGE, (1, 2), ((1, 0),)),
    ('split', LARGE, (1, 2), ((0, 0), (1, 0), (2, 0))),
    ('prof', SMALL, (0,), ((1, 0), (2, 1), (2, 2))),
    ('prof', SMALL, (2, 3), ((1, 0), (2, 1))),
)

# Cells that no option set can launch: cell -> Rule(text, options, big_lut, lands).  `text` quotes the host rule that keeps the cell
# out ("file: condition"); the GPU file asserts it by building `options` (with the long score table if `big_lut`) on `ring`: the
# build fails (`lands` None) or the passes land on the cells `lands` names.  Only what is read from host code belongs here, never a
# cell that was reached and failed.
Rule = collections.namedtuple('Rule', 'text options big_lut lands')
UNREACHABLE = {}


def cells_of(kind, P, geo, fmt, ix):
    """the cells a leg launches unconditionally"""
    modes = tuple(m for m in MODES[kind] if not (m == 9 and fmt == 0))
    return frozenset((P, m, fmt, geo, 1 if kind == 'prof' else 0, ix) for m in modes)


def matrix_of(kind, P, geo):
    """`ring` (2 - 12 entries per row over 4000 columns: every team size cuts it into parts that fit); geometry 3 — the geometry of
    very short rows — takes `short4k`: the rows of `short` (2 - 6 entries) over the same 4000 columns (the 16 000 columns of
    _em_pass_reference's `short` do not fit one or two parts, nor three tables in three)"""
    return 'short4k' if geo == 3 else 'ring'


def rows_of(P, cu_count):
    """rows of `ring` / `short4k` so that EVERY team walks at least STEADY blocks of 64 rows: the kernel deals block t + k T to team t,
    at most cu_count // P teams form, 5 % of the rows are single-entry rows and stay outside the blocks"""
    teams = max(1, cu_count // P)
    return teams, -(-(STEADY + 1) * teams * 64 * 100 // 93)


def options_of(kind, P, geo, fmt, ix):
    o = [('parts', P), ('geometry', geo), ('block_rows', 64), ('value_format', 2 if fmt == 1 else 1)]
    if fmt != 1 and kind != 'split':
        o.append(('index_format', ix))
    o += {'plain': [], 'repro2': [('reproducible', 2)], 'repro1': [('reproducible', 1)], 'lnl4': [('use_likelihood', 1)],
          'split': [('split', 1)], 'prof': [('fused_prof', 1)]}[kind]
    return tuple(o)


def forms_of(kind, fmt):
    """the forms of the lnl pass (option `fused_dbg`) a leg runs: every form of the ladder where the log tables exist; the per-entry
    logarithm and the unforced pass (which is the same kernel then) without them; the unforced pass on the layouts that have one form"""
    if kind != 'plain':
        return (0,)
    if fmt == 1:                                  # 16384 | 32768: the table look-up of log Q, unconditionally (16384 alone leaves the choice armed)
        return (0, 8192, 16384, 32768, 16384 | 32768)
    return (0, 8192, 16384, 32768) if fmt != 0 else (0, 8192)


def _legs():
    out = []
    for kind, teams, geos, pairs in PLAN:
        for P, geo, (fmt, ix) in itertools.product(teams, geos, pairs):
            out.append(Leg('%s-P%d-g%d-f%d-x%d' % (kind, P, geo, fmt, ix), kind, P, geo, fmt, ix, options_of(kind, P, geo, fmt, ix),
                           matrix_of(kind, P, geo), fmt == 0, forms_of(kind, fmt), cells_of(kind, P, geo, fmt, ix)))
    return tuple(out)


LEGS = _legs()


def _shape_leg(leg):
    return leg._replace(name='shape-' + leg.name, options=tuple(kv for kv in leg.options if kv[0] != 'block_rows'), matrix='row_shape')


# The same layouts with the block size left to the library on the row-shape matrix (6000 columns: rows of every length at which a
# kernel changes its path up to 1000 entries, one row of K - 2, register tiles filled to their capacity), for the teams of 4 and of
# 8 of every family (kind, geometry, entry format, index format).  The cells they launch are those of their twins in LEGS.
SHAPE_LEGS = tuple(_shape_leg(leg) for leg in LEGS if leg.P in (4, 8))


def expected_layout(leg):
    """what layout_info(extended=True) must say of the layout a leg forces"""
    want = {'fused': 1, 'P': leg.P, 'geometry': leg.geo, 'value_bytes': 2 if leg.fmt == 1 else 8, 'index_format': leg.ix,
            'index_bytes': {0: 4, 1: 3, 2: 2}[leg.ix], 'split': 1 if leg.kind == 'split' else 0,
            'exact_single': 1 if leg.kind == 'repro1' else 0, 'lnl_fused': 1 if leg.kind == 'lnl4' else 0, 'fallbacks': 0}
    if dict(leg.options).get('block_rows'):
        want['R'] = dict(leg.options)['block_rows']
    return want


def assert_census(leg, census, after):
    """What a leg asserts once its passes have run — census: `Engine.fused_launches()`, after: `layout_info(extended=True)` read after the
    passes.  The kernels launched unconditionally are EXACTLY the leg's cells, nothing fell back, the index format is the leg's, and
    option `reproducible` still guarantees its sums.  (A function of plain values, so tests/test_fused_cells_host.py can show that it
    fails when it should.)"""
    ran = {c for c, (n, _) in census.items() if n > 0}
    assert ran == set(leg.cells), (leg.name, 'launched but not planned', sorted(ran - leg.cells), 'planned but not launched',
                                   sorted(leg.cells - ran))
    assert after['fallbacks'] == 0 and after['index_format'] == leg.ix, (leg.name, after)
    if leg.kind in ('repro1', 'repro2'):
        assert after['reproducible'] in (1, 2), (leg.name, 'a pass gave up moving a grid or a long row made a sum timing-dependent', after)


def kernel_name(cell):
    return 'k_em_fused<%d, %d, %d, %d, %s, %d>' % (cell[0], cell[1], cell[2], cell[3], 'true' if cell[4] else 'false', cell[5])

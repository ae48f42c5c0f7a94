"""The step kernel of the 12-per-CU FP64 build (the headline leg of bench.py) after the stage machine stopped keeping a workspace descriptor
of its own (csrc/fb_step.hpp: d_run / s_run), from the compiler's own figures: tools/resource_report.py compiles the engine to
assembly and prints, per function, instruction count, VGPRs, scratch bytes per lane, scratch loads / stores and occupancy (no GPU needed).
Only those figures are read, no instruction is looked for.

The parent's table (tools/resource_report.py d -DFB_F64_DENSE=1 on a checkout of c197808; profiles/resources_stage_glue.txt):

    function        instr  vgpr scratch  sc_ld  sc_st  occ
    d_solve          1397    70       0      0      0   -1
    d_factor_tail    2156   161       0      0      0   -1
    d_factor         1644   166      12      2      2   -1
    k_fly            3608   168     564     78     46    3

  * k_fly's scratch instructions (sc_ld + sc_st) are not above the parent's 78 + 46 = 124;
  * the step kernel keeps three waves per SIMD;
  * d_factor (which now assembles its right-hand side itself), d_solve and d_factor_tail have no more scratch than they had."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

PARENT = {'d_solve': (0, 0, 0), 'd_factor_tail': (0, 0, 0), 'd_factor': (12, 2, 2)}      # scratch bytes, sc_ld, sc_st at c197808
PARENT_K_FLY_SCRATCH_INSTRUCTIONS = 78 + 46


@pytest.fixture(scope='module')
def table():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'resource_report.py'), 'd', '-DFB_F64_DENSE=1'],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    head = out[0].split()
    assert head[:7] == ['function', 'instr', 'vgpr', 'scratch', 'sc_ld', 'sc_st', 'occ'], head
    rows = {}
    for line in out[1:]:
        p = line.split()
        assert p[0] not in rows, p[0]
        rows[p[0]] = dict(zip(head[1:7], map(int, p[1:7])))
    return rows


def test_step_kernel_scratch_instructions_not_above_the_parent(table):
    r = table['k_fly']
    assert r['sc_ld'] + r['sc_st'] <= PARENT_K_FLY_SCRATCH_INSTRUCTIONS, r


def test_step_kernel_keeps_three_waves_per_simd(table):
    assert table['k_fly']['occ'] == 3, table['k_fly']


@pytest.mark.parametrize('name', list(PARENT))
def test_factor_and_solve_have_no_more_scratch_than_before(table, name):
    r = table[name]; scratch, ld, st = PARENT[name]
    assert r['scratch'] <= scratch and r['sc_ld'] <= ld and r['sc_st'] <= st, r

"""Registers and scratch of the functions on the hot path of the 12-per-CU FP64 build (the headline leg of bench.py), from the compiler's
own figures: tools/resource_report.py compiles the engine to assembly and prints, per function, instruction count, VGPRs, scratch bytes
per lane, scratch loads / stores and occupancy (no GPU needed).  Only those figures are read, no instruction is looked for.

  * d_factor_tail is straight-line code that runs twice per substep: it held the 21 + 6 trunk entries of M and of the damping in every
    lane (54 registers of identical values) and spilled -- 29 scratch stores + 29 reloads, all executed on every call.  One lane per entry
    (fb_smooth.hpp) leaves it without scratch, inside the 168 registers of three waves per SIMD.
  * the 16-row tile instantiation of the Newton solver stays free of scratch with the register hand-over to the noslip passes compiled in.
  * s_constraint_a (the constraint stage around the solver) had 17 scratch loads + 20 stores before the noslip passes were split out of
    d_pgs: not more now.
  * the step kernel keeps three waves per SIMD."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


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


def test_factor_tail_needs_no_scratch(table):
    r = table['d_factor_tail']
    assert r['scratch'] == 0 and r['sc_ld'] == 0 and r['sc_st'] == 0, r
    assert r['vgpr'] <= 168, r


def test_newton_tile_solver_needs_no_scratch(table):
    r = table['d_newton<LDS,LDS,1>']
    assert r['scratch'] == 0 and r['sc_ld'] == 0 and r['sc_st'] == 0, r


def test_constraint_stage_scratch_instructions_not_above_the_parent(table):
    r = table['s_constraint_a']
    assert r['sc_ld'] + r['sc_st'] <= 37, r


def test_step_kernel_occupancy_unchanged(table):
    r = table['k_fly']
    assert r['occ'] == 3 and r['vgpr'] <= 168, r

"""Model variants for domain randomisation: array dicts that differ from a compiled model in real-valued constants only, so that
one batch can step them side by side (engine.ModelGroup, fb_batch_create_group).

The reference randomises one environment at a time -- `template_task(claw_friction=...)`, edits of `physics.model` between episodes;
here the variants are a finite set made on the host, and every environment of a batch carries the index of the one it is stepped with.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Tuple

import numpy as np

from .mjcf_compile import set_const0

# what mj_setConst derives at the reference configuration (mjcf_compile.set_const0) + the two sums that go with it
DERIVED = ('body_subtreemass', 'dof_M0', 'M0_full', 'body_invweight0', 'dof_invweight0', 'tendon_invweight0', 'stat_meaninertia')
SCALES = ('friction_scale', 'mass_scale', 'gain_scale', 'damping_scale', 'stiffness_scale')


def recompute_constants(m: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Recompute, in place, the constants that depend on masses, inertias and frames, as MuJoCo's mj_setConst does: body_subtreemass,
    dof_M0, M0_full, body_ / dof_ / tendon_invweight0 and stat_meaninertia.  On a shipped asset this reproduces them bit for bit."""
    parent = np.asarray(m['body_parent'])
    sub = np.array(m['body_mass'], float)
    for b in range(len(parent) - 1, 0, -1):
        sub[parent[b]] += sub[b]
    m['body_subtreemass'] = sub
    set_const0(m)
    m['stat_meaninertia'] = np.array(float(np.mean(m['dof_M0'])))
    return m


def vary_model(arrays: Mapping[str, np.ndarray], *, friction_scale=1, mass_scale=1, gain_scale=1, damping_scale=1, stiffness_scale=1,
               gravity=None, density=None, viscosity=None) -> Dict[str, np.ndarray]:
    """A new array dict: `arrays` with some real-valued constants changed.  Topology, dimensions, every integer array and the time
    steps stay, so the result is compatible with `arrays` in the sense of engine.ModelGroup.

      friction_scale   sliding friction of every contact pair (pair_friction[:, :2]; geom_friction[:, 0] follows) -- the reference's
                       claw_friction knob, for all geoms; torsional and rolling coefficients stay
      mass_scale       a scalar, or one factor per body ([nbody]; the world body's is ignored): body_mass, and body_inertia by the same
                       factor (a density change).  The constants that depend on them are recomputed as mj_setConst does
                       (recompute_constants).  The fluid-force coefficients (geom_fluid) are geometric and stay.
      gain_scale       actuator_gainprm AND actuator_biasprm together (a scalar or [nu]), so a position actuator (bias = -gain q) stays
                       a position actuator with a stiffer or softer servo
      damping_scale    dof_damping (a scalar or [nv])
      stiffness_scale  jnt_stiffness (a scalar or [njnt])
      gravity          opt_gravity (3-vector), density / viscosity: opt_density / opt_viscosity of the fluid model

    Spring-damper joints (the halteres: the compiler sets their stiffness and damping from the joint's inertia at qpos0) keep their
    COMPILED stiffness and damping under mass_scale -- they are not re-derived from the new inertia; damping_scale and stiffness_scale
    apply to them as to any other joint.  With every scale at 1 and nothing else given the result equals `arrays`."""
    m = {k: np.array(v) for k, v in arrays.items()}
    nbody, nv, nu, njnt = len(m['body_parent']), len(m['dof_bodyid']), len(m['actuator_trntype']), len(m['jnt_type'])

    def factor(x, n, name):
        f = np.asarray(x, float)
        if f.ndim not in (0, 1) or (f.ndim == 1 and f.shape != (n,)):
            raise ValueError(f'{name} must be a scalar or have shape ({n},), got {f.shape}')
        if not np.all(np.isfinite(f)) or np.any(f <= 0):
            raise ValueError(f'{name} must be finite and positive')
        return f

    f = factor(friction_scale, 1, 'friction_scale')
    if np.any(f != 1):
        m['pair_friction'] = m['pair_friction'].astype(float); m['pair_friction'][:, :2] *= f
        if 'geom_friction' in m:
            m['geom_friction'] = m['geom_friction'].astype(float); m['geom_friction'][:, 0] *= f
    f = factor(gain_scale, nu, 'gain_scale')
    if np.any(f != 1):
        col = f[:, None] if f.ndim else f
        m['actuator_gainprm'] = m['actuator_gainprm']*col; m['actuator_biasprm'] = m['actuator_biasprm']*col
    f = factor(damping_scale, nv, 'damping_scale')
    if np.any(f != 1):
        m['dof_damping'] = m['dof_damping']*f
    f = factor(stiffness_scale, njnt, 'stiffness_scale')
    if np.any(f != 1):
        m['jnt_stiffness'] = m['jnt_stiffness']*f
    if gravity is not None:
        g = np.asarray(gravity, float)
        if g.shape != (3,) or not np.all(np.isfinite(g)):
            raise ValueError('gravity must be a finite 3-vector')
        m['opt_gravity'] = g
    for key, val in (('opt_density', density), ('opt_viscosity', viscosity)):
        if val is not None:
            if not np.isfinite(val) or val < 0:
                raise ValueError(f'{key} must be finite and non-negative')
            m[key] = np.array(float(val))
    f = factor(mass_scale, nbody, 'mass_scale')
    if np.any(f != 1):
        fb = np.broadcast_to(f, (nbody,)).copy(); fb[0] = 1.0
        m['body_mass'] = m['body_mass']*fb; m['body_inertia'] = m['body_inertia']*fb[:, None]
        recompute_constants(m)
    return m


def sample_models(arrays: Mapping[str, np.ndarray], n: int, ranges: Mapping[str, Tuple[float, float]], seed: int = 0) -> List[Dict[str, np.ndarray]]:
    """`n` variants of `arrays`, every parameter of `ranges` drawn uniformly from its (low, high): the keys are vary_model's scalar
    keywords (friction_scale, mass_scale, gain_scale, damping_scale, stiffness_scale, density, viscosity).  Reproducible from `seed`."""
    allowed = set(SCALES) | {'density', 'viscosity'}
    bad = set(ranges) - allowed
    if bad:
        raise ValueError(f'unknown parameters {sorted(bad)}; allowed: {sorted(allowed)}')
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(int(n)):
        out.append(vary_model(arrays, **{k: float(rng.uniform(lo, hi)) for k, (lo, hi) in sorted(ranges.items())}))
    return out

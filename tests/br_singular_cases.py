"""Shared by tests/test_br_singular_cpu.py and tests/test_gpu_br_singular.py: states with cells that stand EXACTLY on the
two potentials where Beeler-Reuter's float32 rate formulas are 0/0 (V == -47.0f: alpha_m; V == -23.0f: the second quotient
of i_K1), and on their float32 neighbours.

plane(): the 37 x 53 state of the golden single-step fixture's kind (tests/golden/make_golden.py br_random_state, its own
seed), every drawn potential moved to 0.5 mV clearance from both voltages (tests/test_gpu_timestep.py clear_of_br_singular):
the CONTROL.  Into it are planted float32(-47.0), float32(-23.0) and the +-1, +-2, +-4 float32 neighbours of each

  * in the interior (row 5);
  * on the outer ring (row 0 and column 0): a ring cell's own potential is never read — enforce_boundary replaces it by its
    inner neighbour's — so these cells must come out as control cells do;
  * next to the ring (the neighbours of -47 in row H-2, those of -23 in column W-2): the ring cell beside each is evaluated
    at the planted value, through the boundary clamp along rows and along columns;
  * one exact pair in each corner region of the plane, at (1, 1) and (2, 2) seen from the corner: the first is the exact cell
    next to the ring, read by its two ring neighbours and, clamped along both axes, by the corner cell of the ring.

(58 cells in all see an exact value or a neighbour: the envelope construction of tests/test_gpu_variant_table.py, which
these tests import, refuses a plane with more than 3 % such cells, 58.8 here.)

Cells are classified by the potential the step SEES (the boundary-enforced one), never by where they were planted."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

S47, S23 = np.float32(-47.0), np.float32(-23.0)
OFFSETS = (0, 1, -1, 2, -2, 4, -4)
SHAPE = (37, 53)
HOLE = (25, 17, 7)                  # the phase-field hole of the br_step fixture
DIFF = 0.809
BR_SCALES = [120.0, 1e-5] + [1.0] * 6          # test_br_single_step: V / 120 mV, C / 1e-5, gates / 1
GATE_BOUNDS = (np.float32(0.00001), np.float32(0.99999))
V_BOUNDS = (np.float32(-85.0), np.float32(25.0))


def moved(x, k):
    """the k-th float32 neighbour of x (k < 0: towards -inf)"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


FAMILY47 = [moved(S47, k) for k in OFFSETS]
FAMILY23 = [moved(S23, k) for k in OFFSETS]
NEIGHBOURS = np.array(FAMILY47[1:] + FAMILY23[1:], np.float32)


def seeded_state(H, W, seed=20231):
    """as br_random_state draws it, V at clearance"""
    from test_gpu_timestep import clear_of_br_singular
    rng = np.random.default_rng(seed)
    st = np.empty((8, H, W), np.float32)
    st[0] = rng.uniform(-90.0, 30.0, (H, W))
    st[1] = np.exp(rng.uniform(np.log(1e-7), np.log(1e-5), (H, W)))
    for v in range(2, 8):
        st[v] = rng.uniform(1e-5, 0.99999, (H, W))
    st[0][2, 2:6] = [-85.0, 25.0, -89.99, 29.99]
    st[0] = clear_of_br_singular(st[0])
    return st


def seen(V):
    """the potential a cell's kinetics read: enforce_boundary (ionic.py:107-113)"""
    return np.pad(np.asarray(V, np.float32)[1:-1, 1:-1], 1, mode='edge')


def classify(V):
    """(exact, neighbour) masks of a potential plane, by the boundary-enforced potential"""
    Vs = seen(V)
    exact = (Vs == S47) | (Vs == S23)
    return exact, np.isin(Vs, NEIGHBOURS)


def plane():
    """(state [8, 37, 53] float32 with the planted cells, the control state without them)"""
    H, W = SHAPE
    control = seeded_state(H, W)
    st = control.copy()
    V = st[0]
    both = FAMILY47 + FAMILY23
    for i, x in enumerate(both):
        V[5, 4 + 3 * i] = x                     # interior
        V[0, 4 + 3 * i] = x                     # ring, top row
        V[4 + 2 * i, 0] = x                     # ring, left column
    for i, x in enumerate(FAMILY47[1:]):
        V[H - 2, 6 + 3 * i] = x                 # next to the ring: read by (H-1, c) through the row clamp
    for i, x in enumerate(FAMILY23[1:]):
        V[6 + 2 * i, W - 2] = x                 # next to the ring: read by (r, W-1) through the column clamp
    # corner regions, one exact pair each: the cell both of whose neighbours on the ring AND the corner cell of the ring
    # read it (clamped along both axes), and the cell diagonally inside it.  These are the exact cells next to the ring.
    V[1, 1], V[2, 2] = S47, S23
    V[1, W - 2], V[2, W - 3] = S23, S47
    V[H - 2, 1], V[H - 3, 2] = S23, S47
    V[H - 2, W - 2], V[H - 3, W - 3] = S47, S23
    exact, neigh = classify(V)
    # 12 interior + 12 next to the ring + the 12 ring cells that read those
    # exact: 2 interior + 4 corners x (1 cell read by itself and three ring cells + 1 inside)
    assert int(neigh.sum()) == N_NEIGHBOUR_CELLS and int(exact.sum()) == N_EXACT_CELLS
    return st, control


N_EXACT_CELLS = 22
N_NEIGHBOUR_CELLS = 36          # the ONLY cells of plane() that may be treated by envelope: a count, not a share


def phase(H, W, hole=HOLE):
    """add_hole_to_phase_field of the model classes, without a device"""
    from fib_tf_amd.ionic import IonicModel
    m = IonicModel.__new__(IonicModel)
    m.height, m.width, m.phase, m.defined = H, W, None, False
    m.add_hole_to_phase_field(*hole)
    return m.phase


def step_bounds(rel):
    return [rel * s for s in BR_SCALES]


def on_bound(out):
    """[8, H, W] bool: the value sits on a clip bound (V: -85 / 25; gates: 1e-5 / 0.99999; C has none)"""
    out = np.asarray(out)
    hit = np.zeros(out.shape, bool)
    hit[0] = (out[0] == V_BOUNDS[0]) | (out[0] == V_BOUNDS[1])
    for v in range(2, 8):
        hit[v] = (out[v].astype(np.float32) == GATE_BOUNDS[0]) | (out[v].astype(np.float32) == GATE_BOUNDS[1])
    return hit


def kernel_forms_state(big_br):
    """the 70 x 130 seeded state of tests/test_gpu_timestep.py with every 7th cell of three rows alternately -47.0f and
    -23.0f.  Rows 20 and 21 lie on either side of the seam of the 21-row strip tiles, row 27 opens the second 27-row tile,
    and all three cut the 4-row tiles of the K = 1 kernel at different rows; the column offsets (5, 1, 3 mod 7) put an exact
    cell on columns 54 and 108 (the first column behind a seam of the 54-wide strips), 64 and 127 (either side of the seams
    of the 64-wide tiles) and, stepping by 7 against tiles of 54 and 64 columns, on lanes of every position in between;
    (21, 1) lies next to the ring, whose cell (21, 0) reads it, and (27, 129) on the ring itself, where nobody reads it."""
    st = np.array(big_br, np.float32)
    n = 0
    for row, off in ((20, 5), (21, 1), (27, 3)):
        for c in range(off, st.shape[2], 7):
            st[0][row, c] = S47 if n % 2 == 0 else S23
            n += 1
    return st


def sheet():
    """(state [8, 64, 96], snapped mask): a repolarising plateau.  Rows 0-31: V a ramp from -22 to -24 mV across the columns;
    rows 32-63: from -46 to -48 mV.  One cell in eight (flat index, so the snapped columns shift from row to row) is snapped
    to exactly -23.0f / -47.0f.  Gates at plateau values."""
    H, W = 64, 96
    st = np.empty((8, H, W), np.float32)
    st[0][:32] = np.linspace(-22.0, -24.0, W, dtype=np.float64).astype(np.float32)
    st[0][32:] = np.linspace(-46.0, -48.0, W, dtype=np.float64).astype(np.float32)
    snapped = (np.arange(H * W).reshape(H, W) % 8) == 3
    st[0][:32][snapped[:32]] = S23
    st[0][32:][snapped[32:]] = S47
    for v, x in zip(range(1, 8), (2e-7, 0.9, 1e-5, 1e-5, 0.3, 0.7, 0.2)):      # C M H J D F XI
        st[v] = x
    return st, snapped

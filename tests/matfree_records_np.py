"""NumPy statement of the packed, lane-major element records of the matrix-free passes (csrc/matfree_records.h).

A tile is 64 consecutive elements, one per lane.  Value t of lane l of a sub-record of T values lies at [tile][t][l],
with consecutive t grouped so that a lane's load is 16 bytes (G = 2 doubles or 4 floats); the last group of a
sub-record is as long as what is left.  g: one sub-record of 10 values (g_0, g_1, g_2, det J).  F: NP sub-records of 9
values, NP = 5 (centroid, then the points of vertices 0..3) or NP = 4 (the points of the vertices only).  The last tile
is padded to 64 lanes with copies of the last element."""
import numpy as np

WAVE, G_VALS, F_VALS = 64, 10, 9
G_SOURCE = np.array([0, 1, 2, 4, 5, 6, 8, 9, 10, 3])       # g_0, g_1, g_2, det J in the [16] record


def group(dtype):
    return 16 // np.dtype(dtype).itemsize


def slots_of(E):
    return -(-E // WAVE) * WAVE


def f_slots(NP):
    """points of the [5][10] record the NP sub-records hold"""
    return np.arange(1, 5) if NP == 4 else np.arange(5)


def sub_index(T, G, lane, t):
    q = t // G * G
    return q * WAVE + lane * np.minimum(G, T - q) + (t - q)


def g_index(G, slots):
    """[slots, 10] positions in the packed g buffer"""
    e, t = np.arange(slots)[:, None], np.arange(G_VALS)[None, :]
    return e // WAVE * (G_VALS * WAVE) + sub_index(G_VALS, G, e % WAVE, t)


def f_index(NP, G, slots):
    """[slots, NP, 9] positions in the packed F buffer"""
    e, p, t = np.arange(slots)[:, None, None], np.arange(NP)[None, :, None], np.arange(F_VALS)[None, None, :]
    return (e // WAVE * NP + p) * (F_VALS * WAVE) + sub_index(F_VALS, G, e % WAVE, t)


def pack(gvec, Fq, NP, dtype):
    """gvec [E, 16], Fq [E, 5, 10] in float64 -> (gp, Fp) flat in dtype"""
    E = gvec.shape[0]
    G, slots = group(dtype), slots_of(E)
    src = np.minimum(np.arange(slots), E - 1)               # padding lanes: the last element
    gp, Fp = np.empty(slots * G_VALS, dtype), np.empty(slots * NP * F_VALS, dtype)
    gp[g_index(G, slots)] = gvec[src][:, G_SOURCE].astype(dtype)
    Fp[f_index(NP, G, slots)] = Fq[src][:, f_slots(NP), :F_VALS].astype(dtype)
    return gp, Fp


def unpack(gp, Fp, E, NP):
    """the records the kernel forms: g [E, 4, 3] with g_3 = -((g_0 + g_1) + g_2), det J [E], F [E, 5, 3, 3] with the
    centroid's F = 1/4 ((F_1 + F_2) + (F_3 + F_4)) where it is not stored; and the padding lanes' values as stored"""
    G, slots = group(gp.dtype), slots_of(E)
    g10, F = gp[g_index(G, slots)], Fp[f_index(NP, G, slots)]
    g = np.empty((slots, 4, 3), gp.dtype)
    g[:, :3] = g10[:, :9].reshape(slots, 3, 3)
    g[:, 3] = -((g[:, 0] + g[:, 1]) + g[:, 2])
    F5 = np.empty((slots, 5, F_VALS), Fp.dtype)
    F5[:, f_slots(NP)] = F
    if NP == 4:
        F5[:, 0] = Fp.dtype.type(0.25) * ((F[:, 0] + F[:, 1]) + (F[:, 2] + F[:, 3]))
    return g[:E], g10[:E, 9], F5[:E].reshape(E, 5, 3, 3), (g10[E:], F[E:])

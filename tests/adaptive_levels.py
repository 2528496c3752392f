"""The rule of the multi-level adaptive frame (include/nwe.h: nwe_render_adaptive_levels) restated in numpy float32, on the pieces of
tests/adaptive.py: nested lattices, active cells, render passes, interpolation in the coarsest flat own cell, counts.  Shared by
tests/test_adaptive_levels_host.py and tests/test_gpu_adaptive_levels.py; it reads nothing of the library.

``apply(frame, first_row, k, levels, tol_rgb, tol_depth)`` takes the full frame of ONE pose over the rows of a call, [h, W, 5] with
the channels r, g, b, depth, acc, and returns the frame, the kind map [h, W] (0 level 0 lattice, 1 rendered, 2 interpolated), the
level map [h, W] (kind 0: 0; kind 1: the pass, 1 .. levels; kind 2: the level of the cell interpolated in) and the counts
{pixels, lattice, levels, render_launches, rendered[levels], interpolated[levels]}.  It asserts what makes the rule well defined:
the corners of every classified cell are rendered, a child's parent holds it, and every pixel left finds a flat own cell."""
import numpy as np

from tests import adaptive as A

F = np.float32
INACTIVE, FLAT, BUSY = 0, 1, 2
MAX_LEVELS, MAX_K = 4, 64


def spacing(k, levels, l):
    return k << (levels - 1 - l)


def levels_ok(k, levels):
    return 1 <= k <= MAX_K and 1 <= levels <= MAX_LEVELS and spacing(k, levels, 0) <= MAX_K


def lattices(first, last_excl, k, levels):
    """Per level, coarsest first, the lattice of [first, last_excl) in LOCAL coordinates."""
    return [A.lattice(first, last_excl, spacing(k, levels, l)) - first for l in range(levels)]


def plan(n_poses, rows, width, k, levels):
    """What the planner must size: per-level cells and the most pixels each of the levels + 1 passes can hold."""
    Lh, Lw = lattices(0, rows, k, levels), lattices(0, width, k, levels)
    on = [n_poses * len(Lh[l]) * len(Lw[l]) for l in range(levels)]
    pass_max = [on[0]] + [on[l] - on[l - 1] for l in range(1, levels)] + [n_poses * rows * width - on[-1]]
    return {"pixels": n_poses * rows * width, "lattice": on[0], "list": max(pass_max),
            "cells": [n_poses * len(A.cells(Lh[l])) * len(A.cells(Lw[l])) for l in range(levels)], "pass_max": pass_max}


def apply(frame, first_row, k, levels, tol_rgb, tol_depth):
    assert levels_ok(k, levels)
    frame = np.asarray(frame, dtype=F)
    h, W, _ = frame.shape
    Lh, Lw = lattices(first_row, first_row + h, k, levels), lattices(0, W, k, levels)
    for l in range(1, levels):                          # nested
        assert set(Lh[l - 1]) <= set(Lh[l]) and set(Lw[l - 1]) <= set(Lw[l])
    ch, cw = [A.cells(x) for x in Lh], [A.cells(x) for x in Lw]
    state = [np.full((len(ch[l]), len(cw[l])), INACTIVE, dtype=np.uint8) for l in range(levels)]
    done = np.zeros((h, W), dtype=bool)
    kind = np.full((h, W), A.KIND_INTERPOLATED, dtype=np.uint8)
    level = np.zeros((h, W), dtype=np.uint8)
    done[np.ix_(Lh[0], Lw[0])] = True                   # pass 0
    kind[done] = A.KIND_LATTICE
    rendered, launches = [0] * levels, 1
    for l in range(levels):
        for i, (h0, h1) in enumerate(ch[l]):
            for j, (w0, w1) in enumerate(cw[l]):
                if l > 0:
                    pi, pj = A.cell_of(Lh[l - 1], h0), A.cell_of(Lw[l - 1], w0)
                    (p0, p1), (q0, q1) = ch[l - 1][pi], cw[l - 1][pj]
                    assert p0 <= h0 <= h1 <= p1 and q0 <= w0 <= w1 <= q1                      # the parent holds the child
                    if state[l - 1][pi, pj] != BUSY:
                        continue
                assert done[h0, w0] and done[h0, w1] and done[h1, w0] and done[h1, w1]         # the corners are rendered by now
                is_flat = A.flat([frame[h0, w0], frame[h0, w1], frame[h1, w0], frame[h1, w1]], tol_rgb, tol_depth)
                state[l][i, j] = FLAT if is_flat else BUSY
        if not (state[l] == BUSY).any():
            break                                        # nothing further is launched or classified
        members = np.zeros((h, W), dtype=bool)
        for i, (h0, h1) in enumerate(ch[l]):             # the closed rectangle of every busy cell
            for j, (w0, w1) in enumerate(cw[l]):
                if state[l][i, j] == BUSY:
                    members[h0:h1 + 1, w0:w1 + 1] = True
        if l < levels - 1:
            finer = np.zeros((h, W), dtype=bool)
            finer[np.ix_(Lh[l + 1], Lw[l + 1])] = True
            members &= finer
        members &= ~done
        rendered[l] = int(members.sum())
        launches += 1 if rendered[l] else 0
        kind[members], level[members] = A.KIND_RENDERED, l + 1
        done |= members
    out = frame.copy()
    interpolated = [0] * levels
    for y, x in zip(*np.nonzero(~done)):
        for l in range(levels):
            i, j = A.cell_of(Lh[l], y), A.cell_of(Lw[l], x)
            if state[l][i, j] == FLAT:
                break
            assert state[l][i, j] == BUSY, "own cells nest: an inactive own cell has a flat ancestor"
        else:
            raise AssertionError("a pixel whose own cell of the finest level is busy is rendered")
        (h0, h1), (w0, w1) = ch[l][i], cw[l][j]
        fy = F(0) if h1 == h0 else F(F(y - h0) / F(h1 - h0))
        fx = F(0) if w1 == w0 else F(F(x - w0) / F(w1 - w0))
        for c in range(5):
            top = A.lerp(frame[h0, w0, c], frame[h0, w1, c], fx)
            bottom = A.lerp(frame[h1, w0, c], frame[h1, w1, c], fx)
            out[y, x, c] = A.lerp(top, bottom, fy)
        level[y, x] = l
        interpolated[l] += 1
    counts = {"pixels": h * W, "lattice": len(Lh[0]) * len(Lw[0]), "levels": levels, "render_launches": launches, "rendered": rendered,
              "interpolated": interpolated}
    assert counts["lattice"] + sum(rendered) + sum(interpolated) == h * W
    return out, kind, level, counts


def add_counts(parts):
    """The counts of a pose batch from those of its poses.  The launches are the call's: a pass runs if any pose has pixels in it."""
    total = {"pixels": sum(p["pixels"] for p in parts), "lattice": sum(p["lattice"] for p in parts), "levels": parts[0]["levels"]}
    total["rendered"] = [sum(p["rendered"][l] for p in parts) for l in range(total["levels"])]
    total["interpolated"] = [sum(p["interpolated"][l] for p in parts) for l in range(total["levels"])]
    total["render_launches"] = 1 + sum(1 for n in total["rendered"] if n)
    return total

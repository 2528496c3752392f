"""The rule of the adaptive frame (include/nwe.h: nwe_render_adaptive) restated in numpy float32: lattice, flat cells, kinds,
interpolation, counts.  Shared by tests/test_adaptive_host.py and tests/test_gpu_adaptive.py; it reads nothing of the library.

``apply(frame, first_row, k, tol_rgb, tol_depth)`` takes the full frame of ONE pose over the rows of a call, [h, W, 5] with the
channels r, g, b, depth, acc, and returns the adaptive frame, the kind map [h, W] (0 lattice, 1 rendered, 2 interpolated) and the
counts {pixels, lattice, rendered, interpolated}: a lattice pixel and a rendered one keep the frame's value - the networks give a
pixel the same bits in whatever launch - and an interpolated one is mixed from the four corners of its cell."""
import numpy as np

F = np.float32
KIND_LATTICE, KIND_RENDERED, KIND_INTERPOLATED = 0, 1, 2
FLAG_RGB, FLAG_DEPTH, FLAG_ACC = 1, 2, 4


def lattice(first, last_excl, k):
    """{first + i k < last_excl} and last_excl - 1, ascending."""
    entries = list(range(first, last_excl, k))
    if entries[-1] != last_excl - 1:
        entries.append(last_excl - 1)
    return np.array(entries, dtype=np.int32)


def cells(entries):
    """The (lo, hi) pairs consecutive entries bound; a single entry bounds one degenerate cell."""
    if len(entries) == 1:
        return [(int(entries[0]), int(entries[0]))]
    return [(int(a), int(b)) for a, b in zip(entries[:-1], entries[1:])]


def cell_of(entries, v):
    """min(largest i with entries[i] <= v, cells - 1)"""
    i = int(np.searchsorted(entries, v, side="right")) - 1
    return min(i, len(cells(entries)) - 1)


def lerp(a, b, f):
    """a + (b - a) * f: three float32 operations, each rounded on its own."""
    a, b, f = F(a), F(b), F(f)
    with np.errstate(all="ignore"):
        return F(a + F(F(b - a) * f))


def flat(corners, tol_rgb, tol_depth):
    """corners: four rows (r, g, b, depth, acc).  Every pair, every channel: |v_i - v_j| <= tol; a NaN difference is not."""
    tol = np.array([tol_rgb, tol_rgb, tol_rgb, tol_depth, tol_rgb], dtype=F)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(i + 1, 4):
                d = np.abs((corners[i].astype(F) - corners[j].astype(F)).astype(F))
                if not bool(np.all(d <= tol)):
                    return False
    return True


def apply(frame, first_row, k, tol_rgb, tol_depth):
    frame = np.asarray(frame, dtype=F)
    h, W, _ = frame.shape
    Lh, Lw = lattice(first_row, first_row + h, k) - first_row, lattice(0, W, k)
    ch, cw = cells(Lh), cells(Lw)
    busy = np.zeros((len(ch), len(cw)), dtype=bool)
    for i, (h0, h1) in enumerate(ch):
        for j, (w0, w1) in enumerate(cw):
            busy[i, j] = not flat([frame[h0, w0], frame[h0, w1], frame[h1, w0], frame[h1, w1]], tol_rgb, tol_depth)
    kind = np.full((h, W), KIND_INTERPOLATED, dtype=np.uint8)
    for i, (h0, h1) in enumerate(ch):           # the closed rectangle of every busy cell
        for j, (w0, w1) in enumerate(cw):
            if busy[i, j]:
                kind[h0:h1 + 1, w0:w1 + 1] = KIND_RENDERED
    kind[np.ix_(Lh, Lw)] = KIND_LATTICE
    out = frame.copy()
    for y, x in zip(*np.nonzero(kind == KIND_INTERPOLATED)):
        (h0, h1), (w0, w1) = ch[cell_of(Lh, y)], cw[cell_of(Lw, x)]
        fy = F(0) if h1 == h0 else F(F(y - h0) / F(h1 - h0))
        fx = F(0) if w1 == w0 else F(F(x - w0) / F(w1 - w0))
        for c in range(5):
            top = lerp(frame[h0, w0, c], frame[h0, w1, c], fx)
            bottom = lerp(frame[h1, w0, c], frame[h1, w1, c], fx)
            out[y, x, c] = lerp(top, bottom, fy)
    counts = {"pixels": h * W, "lattice": int((kind == KIND_LATTICE).sum()), "rendered": int((kind == KIND_RENDERED).sum()),
              "interpolated": int((kind == KIND_INTERPOLATED).sum())}
    return out, kind, counts


def interpolation_flags(out, kind):
    """The bits of the non-finite values the interpolation yields."""
    v = out[kind == KIND_INTERPOLATED]
    bad = ~np.isfinite(v)
    return (FLAG_RGB if bad[:, :3].any() else 0) | (FLAG_DEPTH if bad[:, 3].any() else 0) | (FLAG_ACC if bad[:, 4].any() else 0)

"""A numpy restatement of the track overlay's drawing rules (include/stereotrack_vis.h): the
oracle st_draw_tracks equals byte for byte.  Written box by box over whole-image masks - the opposite traversal of the
kernel's, which walks the boxes per pixel.

Rules: coordinates round to the nearest pixel (floor(v + 0.5) in float32); a box with a non-finite coordinate or
x2 < x1 / y2 < y1 paints nothing.  The outline is the outer rectangle [x1 - lw // 2, x2 - lw // 2 + lw - 1] (same in y)
minus the rectangle lw pixels inside it.  The tag starts at (x1 + lw, y1 + lw), (6 L + 1) zoom wide and 9 zoom high for
a label of L characters; font cell (u, v) of the tag holds ink when 1 <= v <= 7 and column (u - 1) % 6 < 5 of glyph
(u - 1) // 6 is set in row v - 1.  Outline, then tag background: out = (a * colour + (256 - a) * pixel + 128) >> 8 with
a = round(alpha * 256); ink is 0 in every plane.  Boxes apply in list order.
"""
import numpy as np

# 5x7 glyphs as text, '#' = ink
_GLYPHS = {
    '0': ('.###.', '#...#', '#..##', '#.#.#', '##..#', '#...#', '.###.'),
    '1': ('..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.'),
    '2': ('.###.', '#...#', '....#', '...#.', '..#..', '.#...', '#####'),
    '3': ('#####', '...#.', '..#..', '...#.', '....#', '#...#', '.###.'),
    '4': ('...#.', '..##.', '.#.#.', '#..#.', '#####', '...#.', '...#.'),
    '5': ('#####', '#....', '####.', '....#', '....#', '#...#', '.###.'),
    '6': ('..##.', '.#...', '#....', '####.', '#...#', '#...#', '.###.'),
    '7': ('#####', '....#', '...#.', '..#..', '.#...', '.#...', '.#...'),
    '8': ('.###.', '#...#', '#...#', '.###.', '#...#', '#...#', '.###.'),
    '9': ('.###.', '#...#', '#...#', '.####', '....#', '...#.', '.##..'),
    ' ': ('.....',) * 7,
    '.': ('.....', '.....', '.....', '.....', '.....', '.##..', '.##..'),
    '|': ('..#..',) * 7,
    '-': ('.....', '.....', '.....', '#####', '.....', '.....', '.....'),
}


def glyph(ch):
    rows = _GLYPHS.get(ch, _GLYPHS[' '])
    return np.array([[c == '#' for c in r] for r in rows], bool)           # (7, 5)


def ref_zoom(xyxy):
    """the reference's adaptive scale on the box area -> the font zoom"""
    x1, y1, x2, y2 = (float(np.float32(v)) for v in xyxy)
    scale = float(np.clip(0.5 + ((y2 - y1) * (x2 - x1) - 800) / (30000 - 800), 0.5, 1.0))
    return max(1, (int(13 * scale) + 3) // 7)


def _round(v):
    return int(np.clip(np.floor(np.float32(v) + np.float32(0.5)), -1048576, 1048576))


def draw_ref(frame, boxes, line_width=3, alpha=0.8):
    """frame: uint8 (3, H, W); boxes: [(xyxy, colour per plane, label str[, zoom])] -> the painted copy."""
    out = frame.astype(np.int64).copy()
    _, H, W = out.shape
    a = int(round(alpha * 256))
    lw, half = int(line_width), int(line_width) // 2
    yy, xx = np.mgrid[0:H, 0:W]

    def blend(mask, colour):
        for p in range(3):
            out[p][mask] = (a * int(colour[p]) + (256 - a) * out[p][mask] + 128) >> 8

    for box in boxes:
        xyxy, colour, label = box[:3]
        if not np.all(np.isfinite(np.asarray(xyxy, np.float32))):
            continue
        x1, y1, x2, y2 = (_round(v) for v in xyxy)
        if x2 < x1 or y2 < y1:
            continue
        zoom = int(box[3]) if len(box) > 3 else ref_zoom(xyxy)
        ox1, oy1, ox2, oy2 = x1 - half, y1 - half, x2 - half + lw - 1, y2 - half + lw - 1
        outer = (xx >= ox1) & (xx <= ox2) & (yy >= oy1) & (yy <= oy2)
        inner = (xx >= ox1 + lw) & (xx <= ox2 - lw) & (yy >= oy1 + lw) & (yy <= oy2 - lw)
        blend(outer & ~inner, colour)
        label = label[:15]
        if not label:
            continue
        L = len(label)
        cells = np.zeros((9, 6 * L + 1), bool)                  # the tag in font cells, margin included
        for i, ch in enumerate(label):
            cells[1:8, 1 + 6 * i:6 + 6 * i] = glyph(ch)
        ink = np.kron(cells, np.ones((zoom, zoom), bool))       # (9 zoom, (6 L + 1) zoom)
        tx, ty = x1 + lw, y1 + lw
        th, tw = ink.shape
        tag = np.zeros((H, W), bool)
        inked = np.zeros((H, W), bool)
        ys, xs = max(ty, 0), max(tx, 0)
        ye, xe = min(ty + th, H), min(tx + tw, W)
        if ys < ye and xs < xe:
            tag[ys:ye, xs:xe] = True
            inked[ys:ye, xs:xe] = ink[ys - ty:ye - ty, xs - tx:xe - tx]
        blend(tag & ~inked, colour)
        for p in range(3):
            out[p][inked] = 0
    return out.astype(np.uint8)

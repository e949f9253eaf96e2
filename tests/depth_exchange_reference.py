"""The depth exchange of a group (gsr_comm_set_depth), restated in numpy from DESIGN.md section 2 ("Exchange buffers") and
section 7 ("Depth in a group") and from nothing else: which samples of the delivered plane a rank owns, where its slab's depth
section lies and what it holds, and how the gathered sections become the plane again.  The plane itself -- which pixels are
sampled, the 16-bit quantiser -- is tests/depth_delivery_reference.py's."""
import numpy as np

BIN_PX = 32
SLAB_FLAG_WORDS = 4
DTYPES = {"f32": np.float32, "u16": np.uint16}


def colour_bytes(slab_w, H):
    """a slab without the option: H rows of slab_w RGBA8 pixels and the flag words"""
    return (slab_w * H + SLAB_FLAG_WORDS) * 4


def slab_width(edges):
    return max(BIN_PX, max(b - a for a, b in edges))


def sample_edges(edges, step):
    """rank q owns the plane's columns [x0 / step, ceil(x1 / step)): x0 is a multiple of 32, so the division is exact.  (An empty
    band -- bands.band_edges hands them to surplus ranks; the library refuses them -- owns nothing.)"""
    out = []
    for a, b in edges:
        assert b <= a or a % BIN_PX == 0
        out.append((a // step, -(-b // step)) if b > a else (-(-a // step),) * 2)
    return out


def layout(W, H, edges, step, fmt):
    """stride (samples per section row: the widest band's, rounded up to 8), offset (of the section in a slab: behind pixels and
    flag words, at the next multiple of 16), section and slab bytes"""
    size = np.dtype(DTYPES[fmt]).itemsize
    sw = slab_width(edges)
    Wd, Hd = -(-W // step), -(-H // step)
    stride = (-(-sw // step) + 7) // 8 * 8
    offset = (colour_bytes(sw, H) + 15) // 16 * 16
    section = Hd * stride * size
    return {"Wd": Wd, "Hd": Hd, "stride": stride, "offset": offset, "section_bytes": section, "slab_bytes": offset + section, "sample_bytes": size}


def section(plane, edges, rank, step, fmt):
    """rank's depth section, [Hd, stride]: its columns of the plane at the front of every row, zeros behind them"""
    plane = np.asarray(plane)
    assert plane.dtype == DTYPES[fmt]
    Hd, Wd = plane.shape
    lay = layout(0, 0, edges, step, fmt)
    a, b = sample_edges(edges, step)[rank]
    b = min(b, Wd)
    out = np.zeros((Hd, lay["stride"]), dtype=plane.dtype)
    if b > a:
        out[:, :b - a] = plane[:, a:b]
    return out


def assemble(sections, Wd, edges, step):
    """the gathered plane from every rank's section; also how many ranks own each sample"""
    Hd = sections[0].shape[0]
    plane = np.zeros((Hd, Wd), dtype=sections[0].dtype)
    owners = np.zeros((Hd, Wd), dtype=np.int32)
    for sec, (a, b) in zip(sections, sample_edges(edges, step)):
        b = min(b, Wd)
        if b > a:
            plane[:, a:b] = sec[:, :b - a]
            owners[:, a:b] += 1
    return plane, owners

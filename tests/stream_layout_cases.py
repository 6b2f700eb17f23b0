"""Files shared by the streamed-layout tests (CPU emulation and GPU): the golden fixtures of the layouts that streamed decompress takes
besides whole interleaved files -- one component, -startbyte / -trunc slices ('Y'), files cut inside their scan -- and one generated
one-component file of several thread segments."""
import functools
import io

import numpy as np

# name -> kind.  `cut`: the file ends inside its scan (a 'Z' file, or a 'Y' slice whose -trunc lies inside the scan)
FIXTURES = {
    "gray_120x88": "gray",
    "rst_rows_gray_64x96": "gray",        # a restart interval per row
    "lay_gray22_80x56": "gray",           # sampling factors 2x2 and padding blocks: two block rows per MCU row, the last one short
    "slice_tail_q97": "slice",
    "slice_rst": "slice",
    "truncated": "cut",
    "truncated_short": "cut",
    "slice_mid_q97": "cut slice",
    "slice_head_cut": "cut slice",
    "slice_4seg_q97": "cut slice",        # four thread segments
}
GENERATED = "gen_gray_2seg"
NOT_STREAMED = ["prog_c420_320x240", "seq_ycb_cr_422_640x480_2seg", "prog_gray_120x88"]
GEN_SIZE = (612, 476)   # 77 x 60 blocks; 604 x 476 (124,660 bytes) still gets one thread segment from the plan for four threads, 612 x 476 two


def generated_gray_jpeg(size=GEN_SIZE):
    """one component (PIL mode "L"), sized so that the thread plan for four threads cuts it into two segments"""
    from PIL import Image

    w, h = size
    rng = np.random.default_rng(1200 + w + h)
    base = np.asarray(Image.fromarray(rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8), dtype=np.uint8), "L").resize((w, h), Image.BICUBIC)).astype(np.int16)
    pic = Image.fromarray(np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8), "L")
    buf = io.BytesIO()
    pic.save(buf, format="JPEG", quality=88)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def generated_gray():
    """(the JPEG, its .lep of at least two thread segments written from the oracle's streams)"""
    import oracle_binding as ob
    from lepton_amd.codec import JpegImage

    jpg = generated_gray_jpeg()
    src = JpegImage(jpg)
    streams, _ = ob.oracle_encode(src.desc, src.plan(4))
    assert len(streams) >= 2
    return jpg, src.write_lep(streams, 4)


def lep_of(name):
    from conftest import golden

    return generated_gray()[1] if name == GENERATED else golden(name)[1]

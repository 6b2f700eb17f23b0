"""The inputs of the refusal tests of `verify` (test_gpu_verify_refuses.py), chosen once and checked on the CPU
(test_verify_tamper_inputs.py): batches of a dozen small golden fixtures cut into three chunks of four, the altered file in the second."""
CHUNK_IMAGES = 4
TARGET = 5     # the altered file's index in the batch: the second file of the second chunk

FILLERS = ["c444_96x80", "lay_440_97x50", "one_block_8x8", "prog_gray_120x88", "c422_128x72", "lay_gray22_80x56", "prog_c444_203x149",
           "q100_64x64", "rst_c420_176x112", "one_col_8x64", "lay_all22_64x48"]

# (fixture, offset into its one stream, xor mask, the oracle's exit code on the stream so altered): offsets in the middle half of the stream,
# as damaged_stream places its damage.  Exit code 0: the oracle decodes the altered stream to its end, into another frame -- only the frame
# comparison can tell.
STREAM_CASES = [
    ("c420_160x120", 2138, 0x01, 7),
    ("c420_160x120", 3200, 0x80, 0),
    ("gray_120x88", 1051, 0x01, 7),
    ("gray_120x88", 1575, 0x01, 0),
    ("prog_c420_320x240", 7807, 0x01, 7),
]

# (fixture, decoded by the GPU scan decoders): the files whose scratch frame is altered -- a baseline file and a one-component file the GPU
# scan decoders take (their Huffman half is checked on the device), and a progressive file cut inside a scan, which the host parser takes
# (its Huffman half is lep_jpeg_check_restores on the host)
SCRATCH_CASES = [("c420_160x120", 1), ("gray_120x88", 1), ("prog_truncated_dc", 0)]


def batch_names(target):
    """the twelve fixtures of a batch around `target`"""
    names = list(FILLERS)
    names.insert(TARGET, target)
    return names

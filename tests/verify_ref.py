"""The three decisions of the round-trip check (lep_batch.hip: lep_compare_kernel, lep_scan_check_kernel, lep_scan_check_bytes_kernel) in
numpy: the plain reference the GPU tests hold the kernels' flag words against.  Flag words are only ever ORed into."""
import numpy as np

PREFIX = 0x80000000   # lep_scan_check.image: the scan a file ends in -- written whole, its first ref_len bytes are the file's


def compare_flags(a, b, nbytes, flags, word, value):
    """lep_compare_kernel: whole 16-byte units of the first nbytes; a difference ORs `value` into flags[word]"""
    n = nbytes // 16 * 16
    out = np.array(flags, dtype=np.uint32)
    if not np.array_equal(np.asarray(a)[:n], np.asarray(b)[:n]):
        out[word] |= np.uint32(value)
    return out


def scan_item_differs(out, out_len, ref, item, bytes_form):
    """one check item (out_off, ref_off, ref_len, image) with its written length: does it set bit 1?"""
    oo, ro, rl, image = item
    if not bytes_form and image & PREFIX:
        if (int(out_len) & 0x7fffffff) < rl:
            return True
    elif int(out_len) != rl:
        return True
    return not np.array_equal(np.asarray(out)[oo:oo + rl], np.asarray(ref)[ro:ro + rl])


def scan_check_flags(out, out_lens, ref, items, flags, bytes_form):
    """lep_scan_check_kernel (bytes_form false) / lep_scan_check_bytes_kernel: the flag words after a launch over `items`"""
    res = np.array(flags, dtype=np.uint32)
    for it, n in zip(items, out_lens):
        if scan_item_differs(out, n, ref, it, bytes_form):
            res[it[3] if bytes_form else it[3] & ~PREFIX] |= np.uint32(2)
    return res

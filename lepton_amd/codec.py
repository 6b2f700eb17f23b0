"""Python mirror of the reference's encoder/decoder interface for the hot path, on top of the C ABI.

Reference interface mirrored (src/lepton/base_coders.hh:26-65):
    BaseEncoder::encode_chunk(const UncompressedComponents*, IOUtil::FileWriter*, const ThreadHandoff*, unsigned)
    BaseDecoder::initialize(DecoderReader*, const std::vector<ThreadHandoff>&) / decode_chunk(UncompressedComponents*)
Here `GpuCodec.encode` takes whole batches of images because on MI355X the unit of parallelism is
(image x thread segment) = one wavefront each, and a useful launch carries hundreds of them.
All computation happens in liblepton_mi355x.so on the GPU; there is no Python or CPU fallback.
"""
import ctypes as C

from . import abi


class LeptonError(RuntimeError):
    """Carries the reference's process exit code (src/vp8/util/memory.hh:13-40)."""

    def __init__(self, code, what):
        super().__init__("%s: exit code %d" % (what, code))
        self.code = code


def _check(rc, what):
    if rc:
        raise LeptonError(rc, what)


class JpegImage:
    """A parsed JPEG: coefficient frame + hand-offs (host memory owned by the library)."""

    def __init__(self, data, allow_progressive=True, start_byte=0, trunc=0, embedding=0):
        """start_byte / trunc: `lepton -startbyte= -trunc=`: the .lep written from this object restores bytes [start_byte, trunc);
        embedding: `lepton -embedding=`: the JPEG starts that many bytes into `data`, the .lep restores all of `data`"""
        self._L = abi.lib()
        self.data = bytes(data[:trunc] if trunc else data)
        self.handle = C.c_void_p()
        if embedding:
            _check(self._L.lep_jpeg_open_embedded(self.data, len(self.data), embedding, C.byref(self.handle)), "lep_jpeg_open_embedded")
        elif start_byte:
            _check(self._L.lep_jpeg_open_slice(self.data, len(self.data), start_byte, C.byref(self.handle)), "lep_jpeg_open_slice")
        else:
            _check(self._L.lep_jpeg_open(self.data, len(self.data), 1 if allow_progressive else 0, C.byref(self.handle)), "lep_jpeg_open")
        self.desc = abi.ImageDesc()
        _check(self._L.lep_jpeg_describe(self.handle, C.byref(self.desc)), "lep_jpeg_describe")

    def plan(self, max_threads=8, image_index=0):
        segs = (abi.Segment * abi.MAX_SEGMENTS)()
        n = self._L.lep_jpeg_plan(self.handle, max_threads, segs, image_index)
        return [segs[i] for i in range(n)]

    def write_lep(self, streams, max_threads=8):
        n = len(streams)
        arr = (abi.Bytes * n)()
        keep = []
        for i, s in enumerate(streams):
            b = C.create_string_buffer(bytes(s), max(1, len(s)))
            keep.append(b)
            arr[i].data = C.cast(b, C.c_void_p).value
            arr[i].len = arr[i].cap = len(s)
        out = abi.Bytes()
        _check(self._L.lep_jpeg_write_lep(self.handle, max_threads, arr, n, C.byref(out)), "lep_jpeg_write_lep")
        data = out.tobytes()
        self._L.lep_free(out.data)
        return data

    def close(self):
        if self.handle:
            self._L.lep_jpeg_close(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LepFile:
    """A parsed .lep: streams + frame geometry; the frame is filled by GpuCodec.decode."""

    def __init__(self, data, prev=None):
        """prev: the previous file of a chained stream of format-version >= 2 files (see lep_stream); it hands over the header
        bytes a `lepton -lepcat` file keeps for its successors"""
        self._L = abi.lib()
        self.data = bytes(data)
        self.handle = C.c_void_p()
        _check(self._L.lep_file_open_next(self.data, len(self.data), prev.handle if prev else None, C.byref(self.handle)), "lep_file_open")
        self.consumed = self._L.lep_file_consumed(self.handle)
        self.more = bool(self._L.lep_chained_file_follows(self.data, len(self.data), self.consumed))
        self.desc = abi.ImageDesc()
        _check(self._L.lep_file_describe(self.handle, C.byref(self.desc)), "lep_file_describe")
        segs = (abi.Segment * abi.MAX_SEGMENTS)()
        st = (abi.Bytes * abi.MAX_SEGMENTS)()
        n = self._L.lep_file_segments(self.handle, segs, st, 0)
        self.segments = [segs[i] for i in range(n)]
        self.streams = [st[i].tobytes() for i in range(n)]

    def recode(self):
        out = abi.Bytes()
        _check(self._L.lep_file_recode(self.handle, C.byref(out)), "lep_file_recode")
        data = out.tobytes()
        self._L.lep_free(out.data)
        return data

    def close(self):
        if self.handle:
            self._L.lep_file_close(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lep_stream(data):
    """the files of a stream of .lep files written back to back (`cat a.lep b.lep | lepton -`, jpgcoder.cc:1868-1897)"""
    data = bytes(data)
    off, prev, out = 0, None, []
    while True:
        f = LepFile(data[off:], prev)
        out.append(f)
        if not f.more:
            return out
        off += f.consumed
        prev = f


class GpuCodec:
    """The MI355X stand-in for VP8ComponentEncoder / VP8ComponentDecoder (one HIP stream, one device)."""

    def __init__(self, device=0):
        self._L = abi.lib()
        self.handle = C.c_void_p()
        rc = self._L.lep_gpu_create(device, C.byref(self.handle))
        if rc:
            raise LeptonError(rc, "lep_gpu_create (no gfx950 device / HIP runtime: there is no CPU fallback)")

    def cut_progressive(self, on=True):
        """lep_gpu_cut_progressive: the batch calls of this codec take progressive files that end inside a scan on the scan kernels"""
        return self._L.lep_gpu_cut_progressive(self.handle, 1 if on else 0)

    def last_error(self):
        return (self._L.lep_gpu_last_error(self.handle) or b"").decode()

    def encode(self, images, plans):
        """images: [JpegImage]; plans: per image list of Segment. Returns per image list of stream bytes."""
        L = self._L
        nimg = len(images)
        descs = (abi.ImageDesc * nimg)(*[im.desc for im in images])
        flat = []
        for i, p in enumerate(plans):
            for s in p:
                flat.append(abi.Segment(i, s.luma_y_start, s.luma_y_end, s.is_last))
        nseg = len(flat)
        segs = (abi.Segment * nseg)(*flat)
        out = (abi.Bytes * nseg)()
        bufs = []
        for k, s in enumerate(flat):
            d = images[s.image].desc
            cap = d.total_blocks() * 160 // max(1, len(plans[s.image])) + d.total_blocks() * 16 + 65536
            b = C.create_string_buffer(cap)
            bufs.append(b)
            out[k].data = C.cast(b, C.c_void_p).value
            out[k].cap = cap
        status = (C.c_int32 * nseg)()
        rc = L.lep_gpu_encode_host(self.handle, descs, nimg, segs, nseg, out, status)
        if rc:
            raise LeptonError(rc, "lep_gpu_encode_host [%s]" % self.last_error())
        res, k = [], 0
        for p in plans:
            res.append([bufs[k + j].raw[: out[k + j].len] for j in range(len(p))])
            k += len(p)
        return res

    def decode(self, files):
        """files: [LepFile]; fills each file's coefficient frame on the GPU."""
        L = self._L
        nimg = len(files)
        descs = (abi.ImageDesc * nimg)(*[f.desc for f in files])
        flat, ins, keep = [], [], []
        for i, f in enumerate(files):
            for s, st in zip(f.segments, f.streams):
                flat.append(abi.Segment(i, s.luma_y_start, s.luma_y_end, s.is_last))
                b = C.create_string_buffer(st, max(1, len(st)))
                keep.append(b)
                ins.append((C.cast(b, C.c_void_p).value, len(st)))
        nseg = len(flat)
        segs = (abi.Segment * nseg)(*flat)
        arr = (abi.Bytes * nseg)()
        for k, (p, n) in enumerate(ins):
            arr[k].data, arr[k].len, arr[k].cap = p, n, n
        status = (C.c_int32 * nseg)()
        rc = L.lep_gpu_decode_host(self.handle, descs, nimg, segs, nseg, arr, status)
        if rc:
            raise LeptonError(rc, "lep_gpu_decode_host [%s]" % self.last_error())

    def decode_rows(self, files, band_mcu_rows, fill=0):
        """files: [LepFile].  A generator over a decode session (lep_gpu_decode_rows_*): after every advance of band_mcu_rows MCU rows
        (<= 0: to the end) the files' coefficient frames are fetched from the device and the list of progress records, one per
        segment in the files' order, is yielded; the frames are readable between yields.  The device frames start filled with the
        byte `fill`.  The session is closed when the generator ends or is closed.  gen.send([indices]) in place of next(gen) retires
        those segments (lep_gpu_decode_rows_retire) before the next advance, whose records it returns: a retired segment has status -2,
        keeps its rows_done and is decoded no further."""
        L, h = self._L, self.handle
        nimg = len(files)
        flat, offs, blob = [], [0], b""
        for i, f in enumerate(files):
            for s, st in zip(f.segments, f.streams):
                flat.append(abi.Segment(i, s.luma_y_start, s.luma_y_end, s.is_last))
                blob += st + bytes(-len(st) % 256)
                offs.append(len(blob))
        nseg = len(flat)
        segs = (abi.Segment * nseg)(*flat)
        lens = (C.c_uint32 * nseg)(*[len(st) for f in files for st in f.streams])
        offsets = (C.c_uint64 * (nseg + 1))(*offs)
        dev = (abi.ImageDesc * nimg)(*[f.desc for f in files])
        owned = []

        def dmalloc(n):
            p = C.c_void_p()
            _check(L.lep_gpu_malloc(h, n, C.byref(p)), "lep_gpu_malloc")
            owned.append(p)
            return p

        begun = False
        try:
            for i, f in enumerate(files):
                for c in range(f.desc.ncomp):
                    p = dmalloc(f.desc.nblocks(c) * 128 + 256)
                    _check(L.lep_gpu_memset(h, p, fill, f.desc.nblocks(c) * 128), "lep_gpu_memset")
                    dev[i].blocks[c] = p.value
            d_streams, d_lens = dmalloc(len(blob) + 256), dmalloc(4 * nseg)
            if blob:
                _check(L.lep_gpu_memcpy_h2d(h, d_streams, blob, len(blob)), "lep_gpu_memcpy_h2d")
            _check(L.lep_gpu_memcpy_h2d(h, d_lens, lens, 4 * nseg), "lep_gpu_memcpy_h2d")
            rc = L.lep_gpu_decode_rows_begin(h, dev, nimg, segs, nseg, d_streams, offsets, d_lens, None)
            if rc:
                raise LeptonError(rc, "lep_gpu_decode_rows_begin [%s]" % self.last_error())
            begun = True
            prog = (abi.DecodeProgress * nseg)()
            running = C.c_int(1)
            while running.value > 0:
                rc = L.lep_gpu_decode_rows_advance(h, band_mcu_rows, prog, C.byref(running))
                if rc:
                    raise LeptonError(rc, "lep_gpu_decode_rows_advance [%s]" % self.last_error())
                for i, f in enumerate(files):
                    for c in range(f.desc.ncomp):
                        _check(L.lep_gpu_memcpy_d2h(h, f.desc.blocks[c], dev[i].blocks[c], f.desc.nblocks(c) * 128), "lep_gpu_memcpy_d2h")
                retire = yield [abi.DecodeProgress.from_buffer_copy(prog[k]) for k in range(nseg)]
                if retire:
                    idx = (C.c_int32 * len(retire))(*retire)
                    rc = L.lep_gpu_decode_rows_retire(h, idx, len(retire))
                    if rc:
                        raise LeptonError(rc, "lep_gpu_decode_rows_retire [%s]" % self.last_error())
        finally:
            if begun:
                L.lep_gpu_decode_rows_end(h)
            for p in owned:
                L.lep_gpu_free(h, p)

    def decompress_stream(self, lep, band_mcu_rows):
        """lep_decompress_stream: (chunks, stats) -- the byte strings the sink received, in order, and the call's statistics as a dict"""
        chunks = []

        def sink(user, data, n):
            chunks.append(C.string_at(data, n))
            return 0

        stats = abi.StreamStats()
        rc = self._L.lep_decompress_stream(self.handle, bytes(lep), len(lep), band_mcu_rows, abi.SINK_FN(sink), None, C.byref(stats))
        if rc:
            raise LeptonError(rc, "lep_decompress_stream [%s]" % self.last_error())
        return chunks, {k: getattr(stats, k) for k, _ in abi.StreamStats._fields_}

    def compress(self, jpg):
        out = abi.Bytes()
        rc = self._L.lep_compress(self.handle, bytes(jpg), len(jpg), C.byref(out))
        if rc:
            raise LeptonError(rc, "lep_compress [%s]" % self.last_error())
        data = out.tobytes()
        self._L.lep_free(out.data)
        return data

    def compress_slice(self, jpg, start_byte, trunc=0):
        out = abi.Bytes()
        _check(self._L.lep_compress_slice(self.handle, jpg, len(jpg), start_byte, trunc, C.byref(out)), "lep_compress_slice")
        data = out.tobytes()
        self._L.lep_free(out.data)
        return data

    def compress_embedded(self, blob, offset):
        out = abi.Bytes()
        _check(self._L.lep_compress_embedded(self.handle, blob, len(blob), offset, C.byref(out)), "lep_compress_embedded")
        data = out.tobytes()
        self._L.lep_free(out.data)
        return data

    def decompress(self, lep):
        out = abi.Bytes()
        rc = self._L.lep_decompress(self.handle, bytes(lep), len(lep), C.byref(out))
        if rc:
            raise LeptonError(rc, "lep_decompress [%s]" % self.last_error())
        data = out.tobytes()
        self._L.lep_free(out.data)
        return data

    def decompress_planes(self, lep, scale=1):
        """lep_decompress_planes: a dict of the record's fields (width, height, ncomp, scale, h_samp, v_samp, plane_width, plane_height,
        pitch) and "planes": one bytes object of pitch * plane_height bytes per component"""
        out = abi.Planes()
        rc = self._L.lep_decompress_planes(self.handle, bytes(lep), len(lep), scale, C.byref(out))
        if rc:
            raise LeptonError(rc, "lep_decompress_planes [%s]" % self.last_error())
        n = out.ncomp
        res = {k: getattr(out, k) for k in ("width", "height", "ncomp", "scale")}
        for k in ("h_samp", "v_samp", "plane_width", "plane_height", "pitch"):
            res[k] = list(getattr(out, k))[:n]
        res["planes"] = [C.string_at(out.plane[c], out.pitch[c] * out.plane_height[c]) for c in range(n)]
        self._L.lep_free(out.plane[0])
        return res

    SAMPLES_MARGIN = 256      # canary bytes in front of and behind every plane of samples()
    SAMPLES_CANARY = 0xEE

    def samples(self, descs, scale=1, rows=None, pitch=None):
        """lep_gpu_samples_device on host frames: descs is a list of ImageDesc with HOST block pointers; the frames go up, the planes are
        laid out in one device buffer filled with SAMPLES_CANARY -- SAMPLES_MARGIN bytes, the plane (pitch * height bytes), SAMPLES_MARGIN
        bytes, for every plane -- and the launch runs.  rows: per image and component (first, end) block rows, None = all; pitch: per
        image and component bytes, None = the plane's width.  Returns per image and component the plane's whole buffer with both
        margins (bytes).  Raises LeptonError with the entry point's code; LeptonError.buffers then holds the buffers as they were left."""
        L, h = self._L, self.handle
        nimg = len(descs)
        dev = (abi.ImageDesc * nimg)()
        owned = []

        def dmalloc(k):
            p = C.c_void_p()
            _check(L.lep_gpu_malloc(h, max(k, 16), C.byref(p)), "lep_gpu_malloc")
            owned.append(p)
            return p

        try:
            planes = (C.c_void_p * (nimg * 3))()
            pitches = (C.c_int32 * (nimg * 3))()
            first = (C.c_int32 * (nimg * 3))()
            end = (C.c_int32 * (nimg * 3))()
            sizes, offs, room = {}, {}, 0
            per = scale if scale in (1, 8) else 1   # (a scale the entry point refuses: the buffers are laid out all the same)
            for i, d in enumerate(descs):
                C.memmove(C.byref(dev[i]), C.byref(d), C.sizeof(abi.ImageDesc))
                for c in range(d.ncomp):
                    k = i * 3 + c
                    nbytes = d.nblocks(c) * 128
                    p = dmalloc(nbytes)
                    _check(L.lep_gpu_memcpy_h2d(h, p, d.blocks[c], nbytes), "h2d")
                    dev[i].blocks[c] = p.value
                    pitches[k] = pitch[i][c] if pitch is not None else d.width_blocks[c] * 8 // per
                    first[k], end[k] = rows[i][c] if rows is not None else (0, d.height_blocks[c])
                    sizes[k] = max(pitches[k], 0) * (d.height_blocks[c] * 8 // per)
                    offs[k] = room + self.SAMPLES_MARGIN
                    room = offs[k] + sizes[k] + self.SAMPLES_MARGIN
            d_out = dmalloc(room)
            _check(L.lep_gpu_memset(h, d_out, self.SAMPLES_CANARY, room), "memset")
            for k, o in offs.items():
                planes[k] = d_out.value + o
            rc = L.lep_gpu_samples_device(h, dev, nimg, scale, first if rows is not None else None, end if rows is not None else None, planes, pitches, None)
            if not rc:
                rc = L.lep_gpu_sync(h)
            host = C.create_string_buffer(room)
            _check(L.lep_gpu_memcpy_d2h(h, host, d_out, room), "d2h")
            raw = host.raw
            bufs = [[raw[offs[i * 3 + c] - self.SAMPLES_MARGIN:offs[i * 3 + c] + sizes[i * 3 + c] + self.SAMPLES_MARGIN] for c in range(d.ncomp)] for i, d in enumerate(descs)]
            if rc:
                e = LeptonError(rc, "lep_gpu_samples_device [%s]" % self.last_error())
                e.buffers = bufs
                raise e
            return bufs
        finally:
            for p in owned:
                L.lep_gpu_free(h, p)

    def decompress_rgb(self, lep):
        """lep_decompress_rgb: a dict of width, height, channels (1 or 3), pitch and "pixels": pitch * height bytes, R,G,B interleaved or
        one byte per pixel"""
        out = abi.Rgb()
        rc = self._L.lep_decompress_rgb(self.handle, bytes(lep), len(lep), C.byref(out))
        if rc:
            raise LeptonError(rc, "lep_decompress_rgb [%s]" % self.last_error())
        res = {k: getattr(out, k) for k in ("width", "height", "channels", "pitch")}
        res["pixels"] = C.string_at(out.pixels, out.pitch * out.height)
        self._L.lep_free(out.pixels)
        return res

    def rgb(self, images):
        """lep_gpu_rgb_device on host planes.  images: a list of dicts with width, height, h_samp, v_samp (lists, one entry per component),
        convert, planes (per component the plane's bytes exactly as they go up, None = no plane), plane_pitch (per component), rgb_pitch and
        optionally rows = (y_first, y_end) (default: every row) and no_output = True (a null output pointer).  The planes go up, the
        outputs are laid out in one device buffer filled with SAMPLES_CANARY -- SAMPLES_MARGIN bytes, the output (rgb_pitch * height bytes),
        SAMPLES_MARGIN bytes, for every image -- and the launch runs.  Returns per image the output's whole buffer with both margins
        (bytes).  Raises LeptonError with the entry point's code; LeptonError.buffers then holds the buffers as they were left."""
        L, h = self._L, self.handle
        nimg = len(images)
        recs = (abi.RgbImage * max(nimg, 1))()
        owned = []

        def dmalloc(k):
            p = C.c_void_p()
            _check(L.lep_gpu_malloc(h, max(k, 16), C.byref(p)), "lep_gpu_malloc")
            owned.append(p)
            return p

        try:
            sizes, offs, room = [], [], 0
            for i, m in enumerate(images):
                r = recs[i]
                r.width, r.height, r.ncomp, r.convert = m["width"], m["height"], m.get("ncomp", len(m["planes"])), 1 if m.get("convert", True) else 0
                for c, plane in enumerate(m["planes"][:3]):
                    r.h_samp[c], r.v_samp[c], r.plane_pitch[c] = m["h_samp"][c], m["v_samp"][c], m["plane_pitch"][c]
                    if plane is not None:
                        raw = bytes(plane)
                        p = dmalloc(len(raw))
                        _check(L.lep_gpu_memcpy_h2d(h, p, raw, len(raw)), "h2d")
                        r.d_plane[c] = p.value
                r.rgb_pitch = m["rgb_pitch"]
                r.y_first, r.y_end = m.get("rows") or (0, m["height"])
                sizes.append(max(r.rgb_pitch, 0) * max(r.height, 0))
                offs.append(room + self.SAMPLES_MARGIN)
                room = offs[i] + sizes[i] + self.SAMPLES_MARGIN
            d_out = dmalloc(room)
            _check(L.lep_gpu_memset(h, d_out, self.SAMPLES_CANARY, room), "memset")
            for i, m in enumerate(images):
                recs[i].d_rgb = None if m.get("no_output") else d_out.value + offs[i]
            rc = L.lep_gpu_rgb_device(h, recs, nimg, None)
            if not rc:
                rc = L.lep_gpu_sync(h)
            host = C.create_string_buffer(max(room, 1))
            _check(L.lep_gpu_memcpy_d2h(h, host, d_out, room), "d2h")
            raw = host.raw
            bufs = [raw[offs[i] - self.SAMPLES_MARGIN:offs[i] + sizes[i] + self.SAMPLES_MARGIN] for i in range(nimg)]
            if rc:
                e = LeptonError(rc, "lep_gpu_rgb_device [%s]" % self.last_error())
                e.buffers = bufs
                raise e
            return bufs
        finally:
            for p in owned:
                L.lep_gpu_free(h, p)

    def _batch(self, fn, blobs, verify, threads, chunk_bytes, chunk_images=0, host_huffman=False):
        n = len(blobs)
        ins = (abi.Bytes * n)()
        keep = []
        for i, b in enumerate(blobs):
            buf = C.create_string_buffer(bytes(b), max(1, len(b)))
            keep.append(buf)
            ins[i].data = C.cast(buf, C.c_void_p).value
            ins[i].len = ins[i].cap = len(b)
        outs = (abi.Bytes * n)()
        status = (C.c_int32 * n)()
        opt = abi.BatchOptions(threads, 1 if verify else 0, chunk_bytes, 1 if host_huffman else 0, chunk_images)
        stats = abi.BatchStats()
        rc = fn(self.handle, ins, n, outs, status, C.byref(opt), C.byref(stats))
        if rc:
            raise LeptonError(rc, "batch pipeline [%s]" % self.last_error())
        res = []
        for i in range(n):
            res.append(outs[i].tobytes() if not status[i] else None)
            if outs[i].data:
                self._L.lep_free(outs[i].data)
        return res, list(status), {k: getattr(stats, k) for k, _ in abi.BatchStats._fields_}

    def compress_batch(self, jpgs, verify=False, threads=0, chunk_bytes=0, chunk_images=0, host_huffman=False, slices=None):
        """[jpeg bytes] -> ([.lep bytes or None], [exit code per file], pipeline statistics); the JPEG Huffman scan decode runs
        on the GPU for eligible files unless host_huffman is set.  slices: one (start_byte, trunc) per file, `lepton -startbyte
        -trunc` ((0, 0) = the whole file); the results are compress_slice's, file by file"""
        if slices is None:
            return self._batch(self._L.lep_compress_batch, jpgs, verify, threads, chunk_bytes, chunk_images, host_huffman)
        if len(slices) != len(jpgs):
            raise ValueError("one (start_byte, trunc) pair per file")
        arr = (abi.Slice * max(1, len(slices)))(*[abi.Slice(int(s), int(t)) for s, t in slices])

        def fn(handle, ins, n, outs, status, opt, stats):
            return self._L.lep_compress_batch_slices(handle, ins, arr, n, outs, status, opt, stats)

        return self._batch(fn, jpgs, verify, threads, chunk_bytes, chunk_images, host_huffman)

    def decompress_batch(self, leps, threads=0, chunk_bytes=0, chunk_images=0, host_huffman=False):
        """[.lep bytes] -> ([jpeg bytes or None], [exit code per file], pipeline statistics); the JPEG Huffman re-encode runs
        on the GPU for eligible files unless host_huffman is set"""
        return self._batch(self._L.lep_decompress_batch, leps, False, threads, chunk_bytes, chunk_images, host_huffman)

    def decompress_batch_stream(self, leps, band_mcu_rows, threads=0):
        """lep_decompress_batch_stream: (pieces, status, stats) -- per file the byte strings its sink calls received, in order, the
        exit code per file, and the call's statistics as a dict"""
        n = len(leps)
        ins = (abi.Bytes * max(1, n))()
        keep = []
        for i, b in enumerate(leps):
            buf = C.create_string_buffer(bytes(b), max(1, len(b)))
            keep.append(buf)
            ins[i].data = C.cast(buf, C.c_void_p).value
            ins[i].len = ins[i].cap = len(b)
        pieces = [[] for _ in range(n)]

        def sink(user, i, data, k):
            pieces[i].append(C.string_at(data, k))
            return 0

        status = (C.c_int32 * max(1, n))()
        opt = abi.BatchOptions(threads, 0, 0, 0, 0)
        stats = abi.BatchStreamStats()
        rc = self._L.lep_decompress_batch_stream(self.handle, ins, n, band_mcu_rows, abi.BATCH_SINK_FN(sink), None, status, C.byref(opt), C.byref(stats))
        if rc:
            raise LeptonError(rc, "lep_decompress_batch_stream [%s]" % self.last_error())
        return pieces, list(status)[:n], {k: getattr(stats, k) for k, _ in abi.BatchStreamStats._fields_}

    def decompress_range(self, lep, first, length=0):
        """lep_decompress_range: the bytes [first, first + length) of decompress(lep) (length 0: to the end), restored from the thread
        segments the range touches"""
        out = abi.Bytes()
        rc = self._L.lep_decompress_range(self.handle, bytes(lep), len(lep), first, length, C.byref(out))
        if rc:
            raise LeptonError(rc, "lep_decompress_range [%s]" % self.last_error())
        data = out.tobytes()
        self._L.lep_free(out.data)
        return data

    def decompress_batch_ranges(self, leps, ranges, band_mcu_rows=0, threads=0):
        """lep_decompress_batch_ranges: ranges = one (first, length) per file (length 0: to the end) -> (outs, status, stats): per file
        the range's bytes or None, the exit code per file, and the call's statistics as a dict.  band_mcu_rows <= 0: bands of
        1, 2, 4, ... MCU rows"""
        n = len(leps)
        if len(ranges) != n:
            raise ValueError("one (first, length) pair per file")
        ins = (abi.Bytes * max(1, n))()
        keep = []
        for i, b in enumerate(leps):
            buf = C.create_string_buffer(bytes(b), max(1, len(b)))
            keep.append(buf)
            ins[i].data = C.cast(buf, C.c_void_p).value
            ins[i].len = ins[i].cap = len(b)
        arr = (abi.Range * max(1, n))(*[abi.Range(int(a), int(b)) for a, b in ranges])
        outs = (abi.Bytes * max(1, n))()
        status = (C.c_int32 * max(1, n))()
        opt = abi.BatchOptions(threads, 0, 0, 0, 0)
        stats = abi.RangeStats()
        rc = self._L.lep_decompress_batch_ranges(self.handle, ins, arr, n, band_mcu_rows, outs, status, C.byref(opt), C.byref(stats))
        if rc:
            raise LeptonError(rc, "lep_decompress_batch_ranges [%s]" % self.last_error())
        res = []
        for i in range(n):
            res.append(outs[i].tobytes() if not status[i] else None)
            if outs[i].data:
                self._L.lep_free(outs[i].data)
        return res, list(status)[:n], {k: getattr(stats, k) for k, _ in abi.RangeStats._fields_}

    def scan_second_chances(self):
        """sequential scans the batch compressor handed to the single-wave kernel since the process started, after the
        lane-per-subsequence scan decoder had answered with a status (process-wide, not per codec object)"""
        return int(self._L.lep_batch_scan_second_chances())

    def debug_write_bins(self, form, parts, chunks, lists, offsets, caps, arena_bytes, guard=0xA5, plan_status=None, part_first=None):
        """lep_gpu_debug_write_bins (tests): the bool writer kernels on `lists` (uint16 arrays, probability | bit << 8), list s into
        [offsets[s], offsets[s] + caps[s]) of an arena of arena_bytes filled with `guard`; part_first: per list the first bins of its
        `parts` parts.  -> (arena, stream_len, status, records): numpy arrays, the records (lists, parts * chunks, 16) uint32 -- None for
        the lane-per-segment form"""
        import numpy as np

        n = len(lists)
        bins = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.uint16) for b in lists] + [np.zeros(1, dtype=np.uint16)]))
        nbins = np.array([len(b) for b in lists], dtype=np.uint32)
        off, cap = np.array(offsets, dtype=np.uint64), np.array(caps, dtype=np.uint32)
        ps = None if plan_status is None else np.array(plan_status, dtype=np.int32)
        pf = None if part_first is None else np.ascontiguousarray(np.array(part_first, dtype=np.uint32).reshape(n, parts))
        K = 0 if form == 0 else (chunks if form == 1 else parts * chunks)
        arena = np.zeros(max(arena_bytes, 1), dtype=np.uint8)
        lens, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        recs = np.zeros((n, K, 16), dtype=np.uint32) if K else None
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = self._L.lep_gpu_debug_write_bins(self.handle, form, parts, chunks, n, p(bins), p(nbins), p(off), p(cap), p(ps), p(pf), guard, p(arena), arena_bytes,
                                              p(lens), p(status), p(recs))
        if rc:
            raise LeptonError(rc, "lep_gpu_debug_write_bins [%s]" % self.last_error())
        return arena[:arena_bytes], lens, status, recs

    def debug_wchunks(self):
        """lep_gpu_debug_wchunks (tests): (parts, chunks, records) of the most recent encode launch -- records a numpy array (segments,
        parts * chunks, 16) uint32 in the caller's segment order; (0, 0, None) when that launch did not use the stitched writer"""
        import numpy as np

        nseg, parts, chunks = C.c_int(), C.c_int(), C.c_int()
        K = self._L.lep_gpu_debug_wchunks(self.handle, None, 0, C.byref(nseg), C.byref(parts), C.byref(chunks))
        if not K:
            return 0, 0, None
        recs = np.zeros((nseg.value, K, 16), dtype=np.uint32)
        if self._L.lep_gpu_debug_wchunks(self.handle, recs.ctypes.data_as(C.c_void_p), nseg.value * K, None, None, None) != K:
            raise LeptonError(1, "lep_gpu_debug_wchunks [%s]" % self.last_error())
        return parts.value, chunks.value, recs

    def _debug_device_arrays(self, arrays):
        """device copies of numpy arrays (lep_gpu_malloc, 16 bytes of room at least) -> (pointers, release)"""
        L, h = self._L, self.handle
        owned = []

        def release():
            for p in owned:
                L.lep_gpu_free(h, p)

        try:
            for a in arrays:
                p = C.c_void_p()
                _check(L.lep_gpu_malloc(h, max(a.nbytes, 16), C.byref(p)), "lep_gpu_malloc")
                owned.append(p)
                if a.nbytes:
                    _check(L.lep_gpu_memcpy_h2d(h, p, a.ctypes.data_as(C.c_void_p), a.nbytes), "lep_gpu_memcpy_h2d")
        except Exception:
            release()
            raise
        return owned, release

    def debug_compare(self, a, b, nbytes, flags, word, value):
        """lep_batch_debug_compare (tests): lep_compare_kernel, as `verify` launches it, on the first nbytes of the uint8 arrays a and b;
        a difference ORs `value` into flags[word].  -> the uint32 flag array as it stands on the device afterwards"""
        import numpy as np

        a, b = np.ascontiguousarray(a, dtype=np.uint8), np.ascontiguousarray(b, dtype=np.uint8)
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        if nbytes > min(a.size, b.size) or not 0 <= word < flags.size:
            raise ValueError("debug_compare: the compared length or the flag word lies outside the arrays")
        (d_a, d_b, d_f), release = self._debug_device_arrays([a, b, flags])
        try:
            rc = self._L.lep_batch_debug_compare(self.handle, d_a, d_b, nbytes, C.c_void_p(d_f.value + 4 * word), value)
            if rc:
                raise LeptonError(rc, "lep_batch_debug_compare [%s]" % self.last_error())
            out = np.zeros_like(flags)
            _check(self._L.lep_gpu_memcpy_d2h(self.handle, out.ctypes.data_as(C.c_void_p), d_f, out.nbytes), "lep_gpu_memcpy_d2h")
            return out
        finally:
            release()

    def debug_scan_check(self, bytes_form, out, out_len, ref, items, flags):
        """lep_batch_debug_scan_check (tests): lep_scan_check_bytes_kernel (bytes_form) or lep_scan_check_kernel on the uint8 arenas
        `out` and `ref`; items = [(out_off, ref_off, ref_len, image)], out_len[i] the written length of item i.  Every item is held
        against the arrays' sizes here: the library call knows none.  -> the uint32 flag array as it stands on the device afterwards"""
        import numpy as np

        out, ref = np.ascontiguousarray(out, dtype=np.uint8), np.ascontiguousarray(ref, dtype=np.uint8)
        out_len, flags = np.ascontiguousarray(out_len, dtype=np.uint32), np.ascontiguousarray(flags, dtype=np.uint32)
        n = len(items)
        if out_len.size != n:
            raise ValueError("debug_scan_check: one written length per item")
        for oo, ro, rl, image in items:
            word = image & ~abi.SCAN_CHECK_PREFIX      # (a prefix item in the bytes form is the library's to refuse)
            if min(oo, ro, rl) < 0 or oo + rl > out.size or ro + rl > ref.size or not 0 <= word < flags.size:
                raise ValueError("debug_scan_check: an item lies outside the arrays")
        arr = (abi.ScanCheck * max(1, n))(*[abi.ScanCheck(*it) for it in items])
        (d_out, d_len, d_ref, d_f), release = self._debug_device_arrays([out, out_len, ref, flags])
        try:
            rc = self._L.lep_batch_debug_scan_check(self.handle, 1 if bytes_form else 0, d_out, d_len, d_ref, arr, n, d_f)
            if rc:
                raise LeptonError(rc, "lep_batch_debug_scan_check [%s]" % self.last_error())
            got = np.zeros_like(flags)
            _check(self._L.lep_gpu_memcpy_d2h(self.handle, got.ctypes.data_as(C.c_void_p), d_f, got.nbytes), "lep_gpu_memcpy_d2h")
            return got
        finally:
            release()

    def debug_tamper(self, where, file, offset, xor_mask):
        """lep_batch_debug_tamper (tests): arms one altered byte for the next compress_batch call (abi.TAMPER_*)"""
        self._L.lep_batch_debug_tamper(where, file, offset, xor_mask)

    def debug_tamper_applied(self):
        return int(self._L.lep_batch_debug_tamper_applied())

    def debug_tamper_seen(self):
        """(flag word, first non-zero status of the verification decode) of the file the last applied alteration was made in"""
        flags, status = C.c_uint32(), C.c_int32()
        self._L.lep_batch_debug_tamper_seen(C.byref(flags), C.byref(status))
        return flags.value, status.value

    def close(self):
        if self.handle:
            self._L.lep_gpu_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

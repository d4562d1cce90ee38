"""Frame ingest / egress around the warp: decoded HWC uint8 frames on the host -> BEV frames, with the
PCIe transfers overlapped with the kernel.

The reference's loop is `ok, img = video.read(); bev = cv2.warpPerspective(img, H, size); writer.write(bev)`
(vis_homo.py:85-111, bev/io/utils.py:124-149): decode, warp and encode strictly one after the other on the host.  Here a
frame travels through three stages that run concurrently on three HIP streams:

    pinned host slot --H2D (copy stream)--> device frame --warp (compute stream)--> device BEV --D2H (copy-back stream)--> pinned host slot

with `depth` slots per stage (default 3), so frame i + 1 uploads and frame i - 1 downloads while frame i is warped; the
link is full duplex.  The decoder can write straight into the next pinned slot (`next_input()`), which removes the host
memcpy a pageable `submit(frame)` needs.  Output is the interleaved BEV frame of the source dtype, or -- `planar=True` --
normalised channel planes (the layout a detector takes; float32, or float16 / bfloat16 with `plane_dtype`), in the same pass.  Results are the resident path's, bit
for bit: the same kernel runs on the same bytes.

`src_format="nv12"`: the host slots take what a video decoder produces -- (H * 3 / 2, W) bytes, the Y plane followed by the rows of (U, V)
pairs -- which halves the upload, and the warp converts each tap to BGR (bev_amd.warp.warp_perspective_nv12; bevwarp_warp_nv12).

`dst_format="nv12"`: the output slots are what a video encoder takes -- (dh * 3 / 2, dw) bytes, the BEV frame's Y plane followed by its rows of
(U, V) pairs -- which halves the download and removes the writer's colour conversion; the warp converts each pixel as it stores it
(bev_amd.warp.warp_perspective_to_nv12, warp_nv12_to_nv12; bevwarp_warp_to_nv12, bevwarp_warp_nv12_to_nv12).

`warp_map=`: a fixed camera's coordinates, lens included, computed once (bev_amd.warp.build_warp_map); every frame is then sampled through
the map, from and into either slot format (bev_amd.warp.remap, remap_nv12, remap_to_nv12, remap_nv12_to_nv12).

SitePipeline is the same ring for a SITE: N fixed cameras in, each through its own warp map, one stitched canvas out -- interleaved, NV12
or normalised channel planes -- with one stitch launch per committed set of frames (bev_amd.warp.remap_stitch and its kin).
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from . import warp as _warp

_hip = None


def _hip_rt():
    """The HIP runtime torch already loaded, bound through ctypes: a frame's eight asynchronous calls (two copies, the
    launch, the events that chain the three streams) cost ~2 us each this way; through torch's stream context managers they
    cost more host time than the transfers take, and the pipeline would be bound by the Python loop."""
    global _hip
    if _hip is None:
        h = ctypes.CDLL("libamdhip64.so")
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        for name, args in (("hipMemcpyAsync", [vp, vp, sz, ctypes.c_int, vp]), ("hipEventCreateWithFlags", [ctypes.POINTER(vp), ctypes.c_uint]),
                           ("hipEventRecord", [vp, vp]), ("hipStreamWaitEvent", [vp, vp, ctypes.c_uint]), ("hipEventSynchronize", [vp]),
                           ("hipEventDestroy", [vp])):
            fn = getattr(h, name)
            fn.restype, fn.argtypes = ctypes.c_int, args
        _hip = h
    return _hip


def _ok(err):
    if err != 0:
        raise _lib.BevWarpError("HIP runtime call failed with error %d" % err)


_H2D, _D2H = 1, 2  # hipMemcpyHostToDevice / hipMemcpyDeviceToHost


def _by_value(v, n):
    """`n` float64 values of a scalar or a sequence (broadcast), in an array of the pipeline's own.  The prepared launches point into it,
    and the library reads through that pointer at every commit(): np.ascontiguousarray alone would hand back a VIEW of a caller's
    contiguous float64 array of that length, and what the caller writes into its array afterwards would reach every later frame."""
    return np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)), dtype=np.float64, order="C")


def _nv12(t, h, w):
    """An NV12 frame in ONE (h * 3 / 2, w) byte buffer, the rows of (U, V) pairs behind the Y rows, as the C ABI takes it: (the Y plane's
    address, the UV plane's), (frame and row stride of Y, frame and row stride of UV)."""
    return (t.data_ptr(), t.data_ptr() + h * w), (0, w, 0, w)


def _buffers(slot):
    """A slot's input buffers (or their byte counts): FramePipeline has one per slot, SitePipeline a list of them (one per camera)."""
    return slot if isinstance(slot, list) else [slot]


class _Ring:
    """What FramePipeline and SitePipeline both stand on: `depth` slots per stage, three private streams (upload, run, download) chained by
    three rings of events, and the raw runtime calls of a slot's way through them -- each written once, here.  A class on it brings
    self.device, depth, download (and zero_copy_out), _launch_py(slot, stream), _prepared(lib) and the nouns of its messages."""

    zero_copy_out = False  # (the kernel stores into the pinned output slot; only FramePipeline has it)
    _nouns = None  # of the "ring is full" message: the class, what is in flight, what is undelivered

    def _allocate(self, in_shapes, in_dtype, out_shape, out_dtype):
        """The pinned and the device slots.  in_shapes: one shape (h_in[slot], d_in[slot] are tensors) or a list of them (lists of tensors)."""
        def inputs(**kw):
            if isinstance(in_shapes, list):
                return [torch.empty(shape, dtype=in_dtype, **kw) for shape in in_shapes]
            return torch.empty(in_shapes, dtype=in_dtype, **kw)

        self.h_in = [inputs(pin_memory=True) for _ in range(self.depth)]
        self.d_in = [inputs(device=self.device) for _ in range(self.depth)]
        self.d_out = [torch.empty(out_shape, dtype=out_dtype, device=self.device) for _ in range(self.depth)]
        self.h_out = [torch.empty(out_shape, dtype=out_dtype, pin_memory=True) for _ in range(self.depth)] if self.download else None

    def _open(self, streams, handles=None):
        """The ring's own state: the three streams (kept alive, and drained by close(); `handles`: what the runtime calls take for them,
        by default the torch streams' raw handles), an empty ring, and 3 * depth events."""
        self._streams = list(streams)
        self.s_up, self.s_run, self.s_down = handles or [ctypes.c_void_p(st.cuda_stream) for st in self._streams]
        self.n_in = 0
        self.pending = collections.deque()  # slots whose results have not been handed out yet
        self.ev_up, self.ev_run, self.ev_down = [], [], []
        self._closed = False  # (from here on close() has streams to drain and events to release, also when the rest of the construction raises)
        hip = _hip_rt()
        for evs in (self.ev_up, self.ev_run, self.ev_down):
            for _ in range(self.depth):
                e = ctypes.c_void_p()
                _ok(hip.hipEventCreateWithFlags(ctypes.byref(e), 2))  # hipEventDisableTiming
                evs.append(e)

    def _start(self, *prepared):
        """The constructors' tail, once the slots are there: the ring, every slot validated once through the Python layer, and one
        prepared launch per slot -- the C ABI call with its arguments bound (`prepared`: what the class's builder takes besides)."""
        self._open([torch.cuda.Stream(self.device) for _ in range(3)])
        for slot in range(self.depth):
            self._launch_py(slot, torch.cuda.current_stream(self.device))
        torch.cuda.synchronize(self.device)
        self._launch = self._prepared(_lib.load(), *prepared)
        nbytes = [t.numel() * t.element_size() for t in _buffers(self.h_in[0])]
        self._in_bytes = nbytes if isinstance(self.h_in[0], list) else nbytes[0]
        self._out_bytes = self.d_out[0].numel() * self.d_out[0].element_size()

    def close(self):
        """Drain the three private streams, then release the events.  The device / pinned buffers were only ever handed to those
        streams as raw addresses (torch does not know they are in use there), so they must not be freed before this."""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        try:
            for st in self._streams:
                st.synchronize()
            hip = _hip_rt()
            for e in self.ev_up + self.ev_run + self.ev_down:
                hip.hipEventDestroy(e)
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    # -- input side
    def next_inputs(self):
        """The pinned host buffers (numpy views) the NEXT frame or set of frames should be decoded into, one per input buffer of the slot
        -- a site: one per camera, (H_k, W_k, 3), or (H_k * 3 / 2, W_k) for NV12; call commit() when they are filled.  Blocks only if that
        slot's previous occupant has not left the device yet."""
        slot = self.n_in % self.depth
        if self.n_in >= self.depth:
            _ok((_hip or _hip_rt()).hipEventSynchronize((self.ev_down if self.download and not self.zero_copy_out else self.ev_run)[slot]))  # its previous occupant is through
        bufs = self.h_in[slot]
        return [t.numpy() for t in bufs] if isinstance(bufs, list) else [bufs.numpy()]

    def commit(self):
        """Upload, launch and (where there is a copy down) download what the next pinned slot holds.  Safe without a next_input(s)() call
        before it: a slot is reused only after its result has been taken (the check below), and result() has then waited for the slot's
        last launch or copy -- the event next_input(s)() waits for as well."""
        if len(self.pending) >= self.depth:  # the slot about to be reused still holds a result nobody has taken
            raise RuntimeError("%s: %d %s are in flight and none has been taken with result(); a ring of depth %d holds at most %d undelivered %s" % (
                self._nouns[0], len(self.pending), self._nouns[1], self.depth, self.depth, self._nouns[2]))
        hip = _hip or _hip_rt()
        slot = self.n_in % self.depth
        self.n_in += 1
        s_up, s_run, ev_up, ev_run = self.s_up, self.s_run, self.ev_up[slot], self.ev_run[slot]
        ds, hs, ns = self.d_in[slot], self.h_in[slot], self._in_bytes
        if isinstance(ns, list):  # (a list of buffers per slot: one upload each)
            for d, h, n in zip(ds, hs, ns):
                _ok(hip.hipMemcpyAsync(d.data_ptr(), h.data_ptr(), n, _H2D, s_up))
        else:
            _ok(hip.hipMemcpyAsync(ds.data_ptr(), hs.data_ptr(), ns, _H2D, s_up))
        _ok(hip.hipEventRecord(ev_up, s_up))
        _ok(hip.hipStreamWaitEvent(s_run, ev_up, 0))
        fn, args = self._launch[slot]
        _lib.check(fn(*args))
        _ok(hip.hipEventRecord(ev_run, s_run))
        if self.download and not self.zero_copy_out:
            s_down = self.s_down
            _ok(hip.hipStreamWaitEvent(s_down, ev_run, 0))
            _ok(hip.hipMemcpyAsync(self.h_out[slot].data_ptr(), self.d_out[slot].data_ptr(), self._out_bytes, _D2H, s_down))
            _ok(hip.hipEventRecord(self.ev_down[slot], s_down))
        self.pending.append(slot)

    # -- output side
    def ready(self):
        return len(self.pending)

    def result(self):
        """The oldest frame's BEV (set's canvas): a numpy view of a pinned slot (download=True; valid until `depth` further ones have been
        committed; bfloat16 planes: the pinned tensor itself) or the device tensor.  Blocks until it is through."""
        slot = self.pending.popleft()
        _ok((_hip or _hip_rt()).hipEventSynchronize((self.ev_down if self.download and not self.zero_copy_out else self.ev_run)[slot]))
        if not self.download:
            return self.d_out[slot]
        h = self.h_out[slot]
        return h if h.dtype == torch.bfloat16 else h.numpy()  # (numpy has no bfloat16)

    def run(self, frames):
        """Generator over an iterable of decoded frames (a site: of N-tuples of them): yields their BEV frames (canvases) in order,
        keeping depth - 1 of them in flight."""
        for f in frames:
            if len(self.pending) >= self.depth - 1:
                yield self.result()
            self.submit(f)
        while self.pending:
            yield self.result()


class FramePipeline(_Ring):
    _nouns = ("FramePipeline", "frames", "frames")

    def __init__(self, src_hw, channels, M, dsize, flags=_warp.INTER_LINEAR, depth=3, dtype=torch.uint8, planar=False, scale=1.0 / 255.0, bias=0.0,
                 download=True, device="cuda", zero_copy_out=True, plane_dtype=torch.float32, src_format="bgr", dst_format="bgr", warp_map=None, map_interpolation=None):
        """src_hw (H, W) of the decoded frames; M the forward homography (as for warpPerspective); dsize (u_size, v_size).
        download=False leaves the BEV frames on the device (results are device tensors valid until `depth` further frames
        have been submitted).  zero_copy_out (with download): the kernel stores the BEV frame straight into the pinned host
        slot over PCIe -- no device copy of it, no D2H copy behind the kernel (on boxes where the two copy directions share an
        engine that copy serialises with the next frame's upload).
        plane_dtype (with planar): torch.float32, torch.float16 or torch.bfloat16 -- the element type of the planes, of the device and
        of the pinned host slots (warp_to_planar's out_dtype).  numpy has no bfloat16: result() hands such a host slot out as a torch
        tensor.
        src_format  "bgr" (default): interleaved (H, W, channels) frames.  "nv12": the input slots are (H * 3 / 2, W) uint8 -- the Y plane,
        then H / 2 rows of (U, V) pairs -- and the output is the BGR BEV frame (or, with dst_format, its NV12 form); channels must be 3, dtype uint8, H and W
        even, and planar output is not available (ValueError).
        dst_format  "bgr" (default): the interleaved BEV frame (or planes, with planar).  "nv12": the device and pinned output slots are
        (dh * 3 / 2, dw) uint8 -- the BEV frame's Y plane, then dh / 2 rows of (U, V) pairs, BT.601 limited range -- from either source
        format, with download on or off and with zero_copy_out; channels must be 3, dtype uint8, dsize even, flags INTER_NEAREST or
        INTER_LINEAR, and planar output is not available (ValueError).  The input frames are taken as B, G, R.
        warp_map    a bev_amd.warp.WarpMap of one frame (build_warp_map: a fixed camera's coordinates, lens included, computed once) on
        `device`: every slot's prepared launch then samples through it (BORDER_CONSTANT, border 0), `M` may be None and `flags` is not
        looked at (the map carries its interpolation).  The launch follows the slots' formats: bevwarp_remap (bgr in, bgr out),
        bevwarp_remap_nv12 (nv12 in, bgr out), bevwarp_remap_to_nv12 (bgr in, nv12 out) or bevwarp_remap_nv12_to_nv12 (nv12 in and out);
        NV12 slots keep their rules above.  With planar it raises ValueError.  None (default): every path above, unchanged.
        map_interpolation   (with warp_map) None (default) or the map's own interpolation: the map's.  INTER_CUBIC with a bilinear map and
        "bgr" slots on both sides: every frame is sampled bicubically through the map (bev_amd.warp.remap(interpolation=INTER_CUBIC)); with
        an NV12 slot on either side, with a nearest map or without warp_map it raises ValueError.
        scale, bias (with planar) are taken by value: the pipeline keeps copies of its own, and the caller's arrays are the caller's again
        once the constructor has returned."""
        if warp_map is not None:
            if not isinstance(warp_map, _warp.WarpMap) or warp_map.n != 1:
                raise ValueError("warp_map must be a bev_amd.warp.WarpMap of one frame, got %s" % (
                    "%d frames" % warp_map.n if isinstance(warp_map, _warp.WarpMap) else type(warp_map).__name__,))
            self._map_interp = _warp._map_interpolation("FramePipeline", warp_map, map_interpolation)
            if self._map_interp != warp_map.interp and (src_format == "nv12" or dst_format == "nv12"):
                raise ValueError("map_interpolation=INTER_CUBIC samples interleaved frames into interleaved frames only: the NV12 samplers have no bicubic")
            if planar:
                raise ValueError("warp_map writes interleaved or NV12 frames only: planar=True is not available with it")
            if warp_map.dsize != (int(dsize[0]), int(dsize[1])):
                raise ValueError("warp_map was built for dsize %s, the pipeline's is %s" % (warp_map.dsize, (int(dsize[0]), int(dsize[1]))))
            if warp_map.device.type != torch.device(device).type:
                raise ValueError("warp_map is on %s, the pipeline runs on %s" % (warp_map.device, device))
        elif map_interpolation is not None:
            raise ValueError("map_interpolation needs a warp_map")
        self.warp_map, self.map_interpolation = warp_map, map_interpolation
        if src_format not in ("bgr", "nv12"):
            raise ValueError("unsupported src_format %r (\"bgr\", \"nv12\")" % (src_format,))
        self.nv12 = src_format == "nv12"
        if self.nv12:
            if planar:
                raise ValueError("src_format=\"nv12\" writes interleaved BGR frames only: planar=True is not available from NV12")
            if int(channels) != 3 or dtype != torch.uint8:
                raise ValueError("src_format=\"nv12\" needs channels=3 and dtype=torch.uint8")
            if int(src_hw[0]) % 2 or int(src_hw[1]) % 2 or int(src_hw[0]) <= 0 or int(src_hw[1]) <= 0:
                raise ValueError("src_format=\"nv12\" needs even frame sides, got %s" % (tuple(src_hw),))
            if warp_map is None and (int(flags) & 7) not in (_warp.INTER_NEAREST, _warp.INTER_LINEAR):
                raise ValueError("src_format=\"nv12\": INTER_NEAREST or INTER_LINEAR")
        if dst_format not in ("bgr", "nv12"):
            raise ValueError("unsupported dst_format %r (\"bgr\", \"nv12\")" % (dst_format,))
        self.nv12_out = dst_format == "nv12"
        if self.nv12_out:
            if planar:
                raise ValueError("dst_format=\"nv12\" writes NV12 frames only: planar=True is not available with it")
            if int(channels) != 3 or dtype != torch.uint8:
                raise ValueError("dst_format=\"nv12\" needs channels=3 and dtype=torch.uint8")
            if int(dsize[0]) % 2 or int(dsize[1]) % 2 or int(dsize[0]) <= 0 or int(dsize[1]) <= 0:
                raise ValueError("dst_format=\"nv12\" needs an even dsize, got %s" % (tuple(dsize),))
            if warp_map is None and (int(flags) & 7) not in (_warp.INTER_NEAREST, _warp.INTER_LINEAR):
                raise ValueError("dst_format=\"nv12\": INTER_NEAREST or INTER_LINEAR")
        if planar and plane_dtype not in _warp._PLANE_DTYPES:
            raise ValueError("unsupported plane_dtype %s (torch.float32, torch.float16, torch.bfloat16)" % (plane_dtype,))
        if depth < 2:
            raise ValueError("depth must be >= 2 (one slot in flight per stage boundary)")
        self.device = torch.device(device)
        self.H, self.W, self.C = int(src_hw[0]), int(src_hw[1]), int(channels)
        self.dw, self.dh = int(dsize[0]), int(dsize[1])
        self.flags, self.depth, self.planar, self.scale, self.bias, self.download = flags, depth, planar, scale, bias, download
        self.plane_dtype = plane_dtype
        self.zero_copy_out = bool(zero_copy_out and download)
        out_shape = (self.C, self.dh, self.dw) if planar else (self.dh, self.dw, self.C)
        if self.nv12_out:
            out_shape = (self.dh * 3 // 2, self.dw)
        self._allocate((self.H * 3 // 2, self.W) if self.nv12 else (self.H, self.W, self.C), dtype, out_shape, plane_dtype if planar else dtype)
        self.minv = None if warp_map is not None else _warp.device_inverse(M, self.device, inverse_given=bool(int(flags) & _warp.WARP_INVERSE_MAP))
        self._start()

    def _prepared(self, lib):
        """[(the C ABI function, its arguments)] per slot.  An NV12 side is one buffer (_nv12); an interleaved side gives its address and
        its frame and row strides -- in bytes, which for the 8-bit entries are their elements."""
        H, W, dh, dw, C, m = self.H, self.W, self.dh, self.dw, self.C, self.warp_map
        interp, nv = int(self.flags) & 7, (self.nv12, self.nv12_out)
        self._keep = [_by_value(self.scale, C), _by_value(self.bias, C)] if self.planar else []  # (host arrays the prepared launches point into)
        launches = []
        for slot in range(self.depth):
            s, d = self.d_in[slot], (self.h_out[slot] if self.zero_copy_out else self.d_out[slot])  # (pinned host memory is device-addressable)
            esz, dsz = s.element_size(), d.element_size()
            src, src_strides = _nv12(s, H, W) if self.nv12 else ((s.data_ptr(),), (s.numel() * esz, s.stride(0) * esz))
            dst, dst_strides = _nv12(d, dh, dw) if self.nv12_out else ((d.data_ptr(),), (d.numel() * dsz, d.stride(0) * dsz))
            head, strides = src + dst + (1, H, W, dh, dw), src_strides + dst_strides
            order = () if all(nv) else (0,)  # (rgb_order 0: the frames on the interleaved side are B, G, R)
            if m is not None:
                maps = m._planes()[:2] + (1,) + m._planes()[2:]
                if any(nv):
                    fn = {(True, True): lib.bevwarp_remap_nv12_to_nv12, (True, False): lib.bevwarp_remap_nv12, (False, True): lib.bevwarp_remap_to_nv12}[nv]
                    args = head + strides + maps + (m.interp, _warp.BORDER_CONSTANT) + order + (None, self.s_run)
                else:
                    fn = lib.bevwarp_remap
                    args = head + (C,) + strides + maps + (_warp._DTYPES[s.dtype], self._map_interp, _warp.BORDER_CONSTANT, None, self.s_run)
            elif any(nv):
                fn = {(True, True): lib.bevwarp_warp_nv12_to_nv12, (True, False): lib.bevwarp_warp_nv12, (False, True): lib.bevwarp_warp_to_nv12}[nv]
                args = head + strides + (self.minv.data_ptr(), 1, interp) + order + (None, self.s_run)
            elif self.planar:
                sc, bi = (a.ctypes.data_as(ctypes.c_void_p) for a in self._keep)
                args = head + (C,) + strides + (d.stride(1) * dsz, self.minv.data_ptr(), 1, _warp._DTYPES[s.dtype], interp, None, sc, bi)
                if self.plane_dtype == torch.float32:
                    fn, args = lib.bevwarp_warp_planar, args + (self.s_run,)
                else:
                    fn, args = lib.bevwarp_warp_planes, args + (_warp._PLANE_DTYPES[self.plane_dtype], self.s_run)
            else:
                fn = lib.bevwarp_warp
                args = head + (C,) + strides + (self.minv.data_ptr(), 1, _warp._DTYPES[s.dtype], interp, None, self.s_run)
            launches.append((fn, args))
        return launches

    def _launch_py(self, slot, stream):
        """The same launch through bev_amd.warp (argument validation; used once per slot at construction)."""
        with torch.cuda.stream(stream):
            if self.warp_map is not None and self.nv12:
                y, uv = _warp.split_nv12(self.d_in[slot])
                (_warp.remap_nv12_to_nv12 if self.nv12_out else _warp.remap_nv12)(y, uv, self.warp_map, out=self.d_out[slot])
            elif self.warp_map is not None and self.nv12_out:
                _warp.remap_to_nv12(self.d_in[slot], self.warp_map, out=self.d_out[slot])
            elif self.warp_map is not None:
                _warp.remap(self.d_in[slot], self.warp_map, out=self.d_out[slot], interpolation=self.map_interpolation)
            elif self.nv12_out and self.nv12:
                y, uv = _warp.split_nv12(self.d_in[slot])
                _warp.warp_nv12_to_nv12(y, uv, None, (self.dw, self.dh), flags=self.flags, out=self.d_out[slot], M_inv_device=self.minv)
            elif self.nv12_out:
                _warp.warp_perspective_to_nv12(self.d_in[slot], None, (self.dw, self.dh), flags=self.flags, out=self.d_out[slot], M_inv_device=self.minv)
            elif self.nv12:
                y, uv = _warp.split_nv12(self.d_in[slot])
                _warp.warp_perspective_nv12(y, uv, None, (self.dw, self.dh), flags=self.flags, out=self.d_out[slot], M_inv_device=self.minv)
            elif self.planar:
                _warp.warp_to_planar(self.d_in[slot], None, (self.dw, self.dh), scale=self.scale, bias=self.bias, flags=self.flags, out=self.d_out[slot],
                                     M_inv_device=self.minv, out_dtype=self.plane_dtype)
            else:
                _warp.warp_perspective(self.d_in[slot], None, (self.dw, self.dh), flags=self.flags, out=self.d_out[slot], M_inv_device=self.minv)

    def next_input(self):
        """The pinned host buffer (numpy view; HWC, or (H * 3 / 2, W) for NV12) the NEXT frame should be decoded into; call commit() when it is filled.
        Blocks only if that slot's previous frame has not left the device yet.  (next_inputs(): the same buffer, in a list of one.)"""
        return self.next_inputs()[0]

    def submit(self, frame):
        """A decoded frame from pageable memory (numpy HWC): copied into the next pinned slot, then committed."""
        buf = self.next_input()
        np.copyto(buf, np.asarray(frame).reshape(buf.shape))
        self.commit()


class SitePipeline(_Ring):
    """FramePipeline's ingest / egress ring for a site of fixed cameras: every committed SET of frames -- one per camera -- is uploaded,
    stitched through the cameras' warp maps into one canvas by ONE launch, and downloaded, on three private streams with `depth` slots
    per stage.  Results are the resident call's (bev_amd.warp.remap_stitch*), bit for bit: the same kernel runs on the same bytes."""

    _nouns = ("SitePipeline", "sets of frames", "results")

    def __init__(self, src_hws, warp_maps, dsize, blend="over", feather=64, border_value=None, depth=3, src_format="bgr", dst_format="bgr", scale=1.0 / 255.0,
                 bias=0.0, plane_dtype=torch.float32, rgb=False, download=True, device="cuda", gains=None):
        """src_hws     (H_k, W_k) of each camera's decoded frames, 1..8 cameras.
        warp_maps   one bev_amd.warp.WarpMap of one frame per camera (build_warp_map: the camera's coordinates, lens included, computed
                    once), all built for `dsize` (u_size, v_size), of one interpolation, on `device`.
        blend, feather, border_value   as bev_amd.warp.remap_stitch: what no camera covers is the border pixel.
        src_format  "bgr": the input slots are (H_k, W_k, 3) uint8 frames.  "nv12": (H_k * 3 / 2, W_k) uint8, the Y plane followed by the
                    rows of (U, V) pairs, as a video decoder delivers them; every H_k and W_k is even.
        dst_format  "bgr": the interleaved (dh, dw, 3) canvas.  "nv12": (dh * 3 / 2, dw) uint8 for a video encoder; dsize is even.
                    "planes": (3, dh, dw) normalised channel planes of plane_dtype (torch.float32, torch.float16 or torch.bfloat16) with
                    scale and bias as bev_amd.warp.remap_stitch_to_planar takes them.
        rgb         NV12 frames into "bgr" or "planes": the result is R, G, B; "bgr" frames into "nv12": the frames are R, G, B.
        download=False leaves the results on the device (valid until `depth` further sets have been committed).
        border_value, scale, bias   taken by value: the pipeline keeps copies of its own, and the caller's arrays are the caller's again
                    once the constructor has returned.
        gains       None, or per-camera exposure gains as bev_amd.warp.remap_stitch takes them ((n_cams,) or (n_cams, 3) floats in
                    [0, 1023/256]; bev_amd.exposure.estimate_gains): the launches then carry BEVWARP_STITCH_GAIN.  set_gains() changes them.
        The launch follows the formats: bevwarp_stitch_maps, bevwarp_stitch_maps_nv12, bevwarp_stitch_maps_to_nv12,
        bevwarp_stitch_maps_nv12_to_nv12, bevwarp_stitch_maps_planes or bevwarp_stitch_maps_nv12_planes."""
        src_hws, warp_maps = [(int(h), int(w)) for h, w in src_hws], list(warp_maps)
        dw, dh = int(dsize[0]), int(dsize[1])
        if len(src_hws) != len(warp_maps):
            raise ValueError("got %d warp maps for %d cameras" % (len(warp_maps), len(src_hws)))
        if not 1 <= len(src_hws) <= _lib.STITCH_MAX_CAMERAS:
            raise ValueError("SitePipeline takes 1..%d cameras, got %d" % (_lib.STITCH_MAX_CAMERAS, len(src_hws)))
        for k, m in enumerate(warp_maps):
            if not isinstance(m, _warp.WarpMap) or m.n != 1:
                raise ValueError("the warp map of camera %d must be a bev_amd.warp.WarpMap of one frame, got %s" % (
                    k, "%d frames" % m.n if isinstance(m, _warp.WarpMap) else type(m).__name__))
            if m.dsize != (dw, dh):
                raise ValueError("the warp map of camera %d was built for dsize %s, the pipeline's is %s" % (k, m.dsize, (dw, dh)))
            if m.device.type != torch.device(device).type:
                raise ValueError("the warp map of camera %d is on %s, the pipeline runs on %s" % (k, m.device, device))
            if m.interp != warp_maps[0].interp:
                raise ValueError("the warp map of camera %d has interpolation %d, camera 0's has %d (one interpolation per site)" % (k, m.interp, warp_maps[0].interp))
        if src_format not in ("bgr", "nv12"):
            raise ValueError("unsupported src_format %r (\"bgr\", \"nv12\")" % (src_format,))
        if dst_format not in ("bgr", "nv12", "planes"):
            raise ValueError("unsupported dst_format %r (\"bgr\", \"nv12\", \"planes\")" % (dst_format,))
        if dst_format == "planes" and plane_dtype not in _warp._PLANE_DTYPES:
            raise ValueError("unsupported plane_dtype %s (torch.float32, torch.float16, torch.bfloat16)" % (plane_dtype,))
        for k, (h, w) in enumerate(src_hws):
            if src_format == "nv12" and (h % 2 or w % 2):
                raise ValueError("src_format=\"nv12\" needs even frame sides, camera %d has %s" % (k, (h, w)))
        if dst_format == "nv12" and (dw % 2 or dh % 2):
            raise ValueError("dst_format=\"nv12\" needs an even dsize, got %s" % ((dw, dh),))
        if depth < 2:
            raise ValueError("depth must be >= 2 (one slot in flight per stage boundary)")
        _warp._stitch_maps_call("SitePipeline", len(src_hws), warp_maps, blend, feather, _warp.BORDER_CONSTANT)  # (the blend and the feather width)
        gain_flag, words = _warp._stitch_gains("SitePipeline", gains, len(src_hws))
        host = {}  # border_value, scale and bias as the prepared launches take them: 3 finite doubles each (border_value: or None)
        for name, v in (("border_value", border_value), ("scale", scale), ("bias", bias)):
            host[name] = None if v is None and name == "border_value" else _by_value(v, 3)
            if host[name] is not None and not np.isfinite(host[name]).all():
                raise ValueError("%s must be finite, got %r" % (name, v))
        self.device = torch.device(device)
        self.src_hws, self.warp_maps, self.dw, self.dh, self.n_cams = src_hws, warp_maps, dw, dh, len(src_hws)
        self.blend, self.feather, self.border_value, self.depth, self.download = blend, int(feather), border_value, depth, download
        self.nv12, self.dst_format, self.scale, self.bias, self.plane_dtype, self.rgb = src_format == "nv12", dst_format, scale, bias, plane_dtype, bool(rgb)
        self.gains = gains
        in_shapes = [(h * 3 // 2, w) if self.nv12 else (h, w, 3) for h, w in src_hws]
        out_shape = {"bgr": (dh, dw, 3), "nv12": (dh * 3 // 2, dw), "planes": (3, dh, dw)}[dst_format]
        out_dtype = plane_dtype if dst_format == "planes" else torch.uint8
        self._allocate(in_shapes, torch.uint8, out_shape, out_dtype)  # (h_in, d_in: [slot][camera])
        self._keep = [host["border_value"], host["scale"], host["bias"]]  # (host arrays the prepared launches point into)
        self._start(gain_flag, words)
        # (`blend` stands behind the interpolation in all six argument lists: set_gains rewrites it)
        self._blend_at = {"nv12": 12, "planes": 10}.get(dst_format, 9 if self.nv12 else 11)
        assert all(args[self._blend_at] == _warp._BLENDS[blend] | gain_flag and args[self._blend_at - 1] == warp_maps[0].interp for _, args in self._launch)

    def _prepared(self, lib, gain_flag, words):
        """[(the C ABI function, its arguments)] per slot, and in _cams the slot's camera table, which the arguments point into."""
        dh, dw, rgb = self.dh, self.dw, int(self.rgb)
        bv, sc, bi = (None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in self._keep)
        blend = (self.warp_maps[0].interp, _warp._BLENDS[self.blend] | gain_flag, self.feather if self.blend == "feather" else 0)
        launches, self._cams = [], []
        for ins, d in zip(self.d_in, self.d_out):
            cams = (_lib.MapCamera * self.n_cams)()
            for cam, s, (h, w), m in zip(cams, ins, self.src_hws, self.warp_maps):
                if self.nv12:
                    (cam.src, cam.uv), (cam.frame_stride, cam.row_stride, cam.uv_frame_stride, cam.uv_row_stride) = _nv12(s, h, w)
                else:
                    cam.src, cam.uv, cam.frame_stride, cam.row_stride = s.data_ptr(), None, s.numel(), s.stride(0)
                cam.src_h, cam.src_w = h, w
                _warp._fill_map_camera(cam, m)
            _warp._set_gain_words(cams, words)
            self._cams.append(cams)
            head = (ctypes.addressof(cams), self.n_cams)
            if self.dst_format == "nv12":
                dst, strides = _nv12(d, dh, dw)
                args = head + dst + (1, dh, dw) + strides + blend
                if self.nv12:
                    launches.append((lib.bevwarp_stitch_maps_nv12_to_nv12, args + (bv, self.s_run)))
                else:
                    launches.append((lib.bevwarp_stitch_maps_to_nv12, args + (rgb, bv, self.s_run)))
            elif self.dst_format == "planes":
                psz = d.element_size()
                args = head + (d.data_ptr(), 1, dh, dw, d.numel() * psz, d.stride(0) * psz, d.stride(1) * psz) + blend
                tail = (bv, sc, bi, _warp._PLANE_DTYPES[self.plane_dtype], self.s_run)
                if self.nv12:
                    launches.append((lib.bevwarp_stitch_maps_nv12_planes, args + (rgb,) + tail))
                else:
                    launches.append((lib.bevwarp_stitch_maps_planes, args + tail))
            elif self.nv12:
                args = head + (d.data_ptr(), 1, dh, dw, d.numel(), d.stride(0)) + blend + (rgb, _warp.BORDER_CONSTANT, bv, self.s_run)
                launches.append((lib.bevwarp_stitch_maps_nv12, args))
            else:
                args = head + (d.data_ptr(), 1, dh, dw, 3, d.numel(), d.stride(0), _lib.U8) + blend + (_warp.BORDER_CONSTANT, bv, self.s_run)
                launches.append((lib.bevwarp_stitch_maps, args))
        return launches

    def set_gains(self, gains):
        """New per-camera gains (as the constructor's `gains`; None: none) for every set of frames committed from now on: the gain words
        in every slot's host camera table and the flag in its `blend` word are rewritten.  The library reads the table during the call
        only and takes the gains by value, so sets already committed keep the gains they were committed with, and the next commit()
        uses the new ones.  Call it from the thread that commits."""
        gain_flag, words = _warp._stitch_gains("SitePipeline.set_gains", gains, self.n_cams)
        blend_id = _warp._BLENDS[self.blend] | gain_flag
        for slot, (fn, args) in enumerate(self._launch):
            _warp._set_gain_words(self._cams[slot], words or [0] * self.n_cams)
            self._launch[slot] = (fn, args[:self._blend_at] + (blend_id,) + args[self._blend_at + 1:])
        self.gains = gains

    def _launch_py(self, slot, stream):
        """The same launch through bev_amd.warp (argument validation; used once per slot at construction)."""
        kw = dict(blend=self.blend, feather=self.feather, border_value=self.border_value, out=self.d_out[slot], gains=self.gains)
        with torch.cuda.stream(stream):
            if self.nv12:
                ys, uvs = zip(*[_warp.split_nv12(t) for t in self.d_in[slot]])
                if self.dst_format == "nv12":
                    _warp.remap_stitch_nv12_to_nv12(ys, uvs, self.warp_maps, **kw)
                elif self.dst_format == "planes":
                    _warp.remap_stitch_nv12_to_planar(ys, uvs, self.warp_maps, scale=self.scale, bias=self.bias, rgb=self.rgb, out_dtype=self.plane_dtype, **kw)
                else:
                    _warp.remap_stitch_nv12(ys, uvs, self.warp_maps, rgb=self.rgb, **kw)
            elif self.dst_format == "nv12":
                _warp.remap_stitch_to_nv12(self.d_in[slot], self.warp_maps, rgb=self.rgb, **kw)
            elif self.dst_format == "planes":
                _warp.remap_stitch_to_planar(self.d_in[slot], self.warp_maps, scale=self.scale, bias=self.bias, out_dtype=self.plane_dtype, **kw)
            else:
                _warp.remap_stitch(self.d_in[slot], self.warp_maps, **kw)

    def submit(self, frames):
        """One decoded frame per camera from pageable memory (numpy): copied into the next pinned slots, then committed."""
        bufs = self.next_inputs()
        if len(frames) != len(bufs):
            raise ValueError("got %d frames for %d cameras" % (len(frames), len(bufs)))
        for buf, frame in zip(bufs, frames):
            np.copyto(buf, np.asarray(frame).reshape(buf.shape))
        self.commit()

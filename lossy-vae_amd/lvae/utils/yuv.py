"""YUV frames in and out of the codec: planes of raw video <-> the fp32 NCHW RGB tensors in [0, 1] the models code, and raw .yuv files.

One implementation behind two sets of names.  The general one is `YuvFrame`: planar, 8 / 10 / 12 bits, 4:2:0 / 4:2:2 / 4:4:4, chroma sited
in the centre or on the left (co-sited, H.264 / HEVC chroma_sample_loc_type 0), BT.601 / BT.709 / BT.2020 non-constant luminance
(`yuv_to_rgb_expr2`, `rgb_to_yuv_expr2`, `to_rgb01_any`, `from_rgb01_any`, `read_yuv`, `write_yuv`).  The 8-bit 4:2:0 API (`Yuv420Frame`:
planar I420 / semi-planar NV12 bytes, centre-sited chroma, BT.601 / BT.709; `yuv_to_rgb_expr`, `rgb_to_yuv_expr`, `to_rgb01`, `from_rgb01`,
`read_yuv420`, `write_yuv420`) is the general one at depth 8, '420', 'center' with its own frame class and argument checks.

This file DEFINES the conversions, as torch expressions on CPU tensors: fp32 throughout, the constants below as fp32 values, every
operation rounded on its own, divisions IEEE.  On the GPU the conversions are the HIP kernels of csrc/yuv_io.hip, which reproduce the
expressions' bits: a frame is uploaded as the bytes its file held (1 or 2 per sample), upsampled, converted and replicate-padded where
the encoder reads it, and a reconstruction becomes codes on the device before it is copied back.  The same split as
utils.image.to_float01 / to_u8.

Samples of more than 8 bits are 16-bit little-endian words with the value in the LOW bits (yuv420p10le, yuv422p12le: what ffmpeg rawvideo
and HM / VTM read and write), held as torch.int16.  The frames hardware video decoders deliver are a third kind, `YuvSpFrame`: semi-planar,
10 / 12 bits at 4:2:0 / 4:2:2 (P010, P012, P210, P212), a luma plane and ONE plane of interleaved U V words with the value in the HIGH bits
(`read_yuv_sp`, `write_yuv_sp`, `YuvSpBatch`; `YuvSpFrame.to_planar` / `YuvFrame.to_semiplanar` state the layout as torch ops).  Their
conversion IS the planar one -- the SP variants of csrc/yuv_io.hip give the bits the planar kernels give for the deinterleaved, shifted
planes -- so yuv_to_rgb_expr2 / rgb_to_yuv_expr2 define it too.  Not supported: 16-bit depth (P016), chroma sitings other than centre / left,
8-bit semi-planar 4:2:2 / 4:4:4 (NV16 / NV24).  The colour parameters, the depth and the siting are the caller's on both sides: no stream
stores them; the sequence container of utils/yuvseq.py does.

What the three frame classes differ in is one value, `FrameFormat(layout, depth, subsampling)`: it reads, allocates, crops and batches
frames of its kind, `to_rgb01_any` / `from_rgb01_any` take every kind through it (`to_rgb01` / `from_rgb01` forward to them), and which
layout exists at which depth, subsampling, siting and matrix is the rule of utils.yuvseq.check_layout, stated nowhere else.

`to_rgb01_scaled` / `from_rgb01_scaled` / `ScaledYuvBatch` are the two conversions with the resampler of utils/resample.py between them and
the planes, each as ONE kernel (csrc/resample_yuv.hip) with the bits of the composition: frames coded at reduced resolution.

`stitch_tiles_yuv` (the end of the file) writes a frame, or a window of one, straight from the decoded tiles of a tiled image
(csrc/tile_stitch_yuv.hip): utils.image.stitch_tiles and from_rgb01_any as one kernel, with their bits.
"""
import ctypes
import math
import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from .image import _canvas
from .yuvseq import _extent_ok, check_layout

from .._native import YUV_CHROMA as CHROMA, YUV_FORMATS as FORMATS, YUV_MATRICES as MATRICES, YUV_RANGES as RANGES   # index = LVAE_YUV_* code
from .._native import YUV_DEPTHS as DEPTHS, YUV_MATRICES2 as MATRICES2, YUV_SITINGS as SITINGS, YUV_SUBSAMPLINGS as SUBSAMPLINGS
from .._native import YUV_LAYOUTS as LAYOUTS                 # LVAE_YUV_LAYOUT_*
# per matrix: Kr, Kg, Kb, a = 2(1 - Kr), b = 2(1 - Kb), d = 2 Kb (1 - Kb) / Kg, e = 2 Kr (1 - Kr) / Kg -- the literals of csrc/yuv_io.hip
COEF = {'bt601': (0.299, 0.587, 0.114, 1.402, 1.772, 0.344136286, 0.714136286),
        'bt709': (0.2126, 0.7152, 0.0722, 1.5748, 1.8556, 0.187324273, 0.468124273),
        'bt2020': (0.2627, 0.678, 0.0593, 1.4746, 1.8814, 0.164553127, 0.571353127)}    # YuvFrame API only (MATRICES2)
SCALES = {'limited': (16.0, 219.0, 224.0), 'full': (0.0, 255.0, 255.0)}       # luma offset, luma scale, chroma scale


def _check(matrix, range, chroma='bilinear', fmt='i420'):
    for v, known, what in ((matrix, MATRICES, 'matrix'), (range, RANGES, 'range'), (chroma, CHROMA, 'chroma'), (fmt, FORMATS, 'fmt')):
        if v not in known:
            raise ValueError(f'{what} is one of {known}, got {v!r}')


class Yuv420Frame:
    """One 8-bit 4:2:0 frame: `fmt` 'i420' with planes y (h, w), u, v (h/2, w/2), or 'nv12' with y (h, w) and uv (h/2, w/2, 2) -- uint8
    tensors on one device (numpy arrays become CPU tensors).  `u` / `v` of an NV12 frame are strided views of `uv`.  h and w are even."""

    def __init__(self, fmt, y, u=None, v=None, uv=None):
        if fmt not in FORMATS:
            raise ValueError(f'fmt is one of {FORMATS}, got {fmt!r}')
        t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)))
        y, u, v, uv = t(y), t(u), t(v), t(uv)
        if y is None or y.dim() != 2 or y.dtype != torch.uint8:
            raise ValueError('y is an (h, w) uint8 plane')
        h, w = int(y.shape[0]), int(y.shape[1])
        if h <= 0 or w <= 0 or h % 2 or w % 2:
            raise ValueError(f'a 4:2:0 frame has even, positive sides, got {h} x {w}')
        if fmt == 'i420':
            if uv is not None or any(p is None or p.dtype != torch.uint8 or tuple(p.shape) != (h // 2, w // 2) or p.device != y.device for p in (u, v)):
                raise ValueError(f'i420: u and v are ({h // 2}, {w // 2}) uint8 planes on the device of y')
        else:
            if u is not None or v is not None or uv is None or uv.dtype != torch.uint8 or tuple(uv.shape) != (h // 2, w // 2, 2) or uv.device != y.device:
                raise ValueError(f'nv12: uv is an ({h // 2}, {w // 2}, 2) uint8 plane on the device of y')
            u, v = uv[..., 0], uv[..., 1]
        self.fmt, self.y, self.u, self.v, self.uv, self.h, self.w = fmt, y, u, v, uv, h, w

    @property
    def device(self):
        return self.y.device

    @property
    def size(self):
        return (self.h, self.w)

    def planes(self):
        """The planes as the file holds them: (y, u, v) or (y, uv)."""
        return (self.y, self.u, self.v) if self.fmt == 'i420' else (self.y, self.uv)

    def to(self, device, non_blocking=False):
        if torch.device(device) == self.device:
            return self
        mv = lambda p: p.to(device, non_blocking=non_blocking)
        return Yuv420Frame('i420', mv(self.y), mv(self.u), mv(self.v)) if self.fmt == 'i420' else Yuv420Frame('nv12', mv(self.y), uv=mv(self.uv))

    def cpu(self):
        return self.to('cpu')

    def as_format(self, fmt):
        """The same samples in the other plane layout (a copy of the chroma) or, for its own format, the frame itself."""
        if fmt == self.fmt:
            return self
        if fmt == 'nv12':
            return Yuv420Frame('nv12', self.y, uv=torch.stack([self.u, self.v], -1))
        return Yuv420Frame('i420', self.y, self.u.contiguous(), self.v.contiguous())


def frame_bytes(width, height):
    return FrameFormat('i420').frame_bytes(width, height)


def _read_raw(path, per, frames, start, who):
    """Frames `start` .. of a raw file of `per` bytes per frame (all of them, or the first `frames`) -> a list of uint8 views, one per
    frame, of ONE buffer -- pinned when a GPU is there, so a frame's upload is an asynchronous copy.  ValueError: a file size that is
    not a whole number of frames, no frame in the range, a short read."""
    size = os.path.getsize(path)
    if size == 0 or size % per:
        raise ValueError(f'{who}: {path} holds {size} bytes, not a whole number of frames of {per} bytes')
    n = size // per - int(start) if frames is None else min(int(frames), size // per - int(start))
    if n <= 0 or start < 0:
        raise ValueError(f'{who}: frames={frames}, start={start} of {size // per}')
    buf = torch.empty(n * per, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    with open(path, 'rb') as f:
        f.seek(int(start) * per)
        got = f.readinto(buf.numpy())
    if got != n * per:
        raise ValueError(f'{who}: short read of {path}')
    return [buf[i * per:(i + 1) * per] for i in range(n)]


def read_yuv420(path, width, height, fmt='i420', frames=None, start=0):
    """A raw .yuv file of `width` x `height` 8-bit 4:2:0 frames -> list of Yuv420Frame on the CPU (all of them, or the first `frames`; from frame `start` on).
    The file is read into ONE buffer -- pinned when a GPU is there, so a frame's upload is an asynchronous copy -- and the planes are
    views of it.  ValueError: odd or non-positive sides, a file size that is not a whole number of frames, an unknown fmt."""
    _check('bt709', 'limited', fmt=fmt)
    if width <= 0 or height <= 0 or width % 2 or height % 2:
        raise ValueError(f'read_yuv420: a 4:2:0 frame has even, positive sides, got {width} x {height}')
    return FrameFormat(fmt).read(path, width, height, frames, start, 'read_yuv420')


# =============================================================================================== 8 / 10 / 12 bits, 4:2:0 / 4:2:2 / 4:4:4
SHIFTS = {'420': (1, 1), '422': (1, 0), '444': (0, 0)}       # subsampling -> (horizontal, vertical) shift of the chroma planes


def _check2(depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', chroma='bilinear'):
    for v, known, what in ((depth, DEPTHS, 'depth'), (subsampling, SUBSAMPLINGS, 'subsampling'), (siting, SITINGS, 'siting'),
                           (matrix, MATRICES2, 'matrix'), (range, RANGES, 'range'), (chroma, CHROMA, 'chroma')):
        if v not in known:
            raise ValueError(f'{what} is one of {known}, got {v!r}')


class YuvFrame:
    """One planar frame of `depth` 8 | 10 | 12 bits at `subsampling` '420' | '422' | '444': planes y (h, w) and u, v of (h/2, w/2), (h, w/2)
    or (h, w) on one device -- torch.uint8 at depth 8, torch.int16 above it: the 16 bits of the container with the value in the LOW bits,
    as in yuv420p10le / yuv422p12le.  numpy arrays become CPU tensors (uint16 arrays are reinterpreted, not copied).  Both sides are even
    for 4:2:0, the width for 4:2:2.  A CPU frame with a code outside 0 .. 2^depth - 1 raises ValueError; frames on a device are not scanned:
    the kernels mask every sample they read to `depth` bits (as does the defining expression).  scan=False: nor is this one, whose planes
    are yet to be written."""

    def __init__(self, y, u, v, depth=8, subsampling='420', scan=True):
        _check2(depth, subsampling)

        def t(a):
            if isinstance(a, torch.Tensor):
                return a
            a = np.asarray(a)
            return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
        y, u, v = t(y), t(u), t(v)
        dtype = torch.uint8 if depth == 8 else torch.int16
        if y.dim() != 2 or y.dtype != dtype:
            raise ValueError(f'y is an (h, w) {dtype} plane at depth {depth}, got {tuple(y.shape)} {y.dtype}')
        h, w = int(y.shape[0]), int(y.shape[1])
        if not _extent_ok(h, w, subsampling):
            raise ValueError(f'a {subsampling} frame has positive sides, even where the chroma is subsampled, got {h} x {w}')
        sx, sy = SHIFTS[subsampling]
        cs = (h >> sy, w >> sx)
        if any(p.dtype != dtype or tuple(p.shape) != cs or p.device != y.device for p in (u, v)):
            raise ValueError(f'u and v are {cs} {dtype} planes on the device of y')
        if scan and depth > 8 and y.device.type == 'cpu':
            for name, p in zip('yuv', (y, u, v)):
                if int(p.min()) < 0 or int(p.max()) > (1 << depth) - 1:
                    raise ValueError(f'plane {name} holds codes outside 0 .. {(1 << depth) - 1} (the value belongs in the low {depth} bits)')
        self.y, self.u, self.v, self.depth, self.subsampling, self.h, self.w = y, u, v, depth, subsampling, h, w

    @property
    def device(self):
        return self.y.device

    @property
    def size(self):
        return (self.h, self.w)

    def planes(self):
        """The planes in file order: (y, u, v)."""
        return (self.y, self.u, self.v)

    def to(self, device, non_blocking=False):
        if torch.device(device) == self.device:
            return self
        fr = YuvFrame.__new__(YuvFrame)                      # (the planes were checked when this frame was made)
        fr.__dict__.update(self.__dict__)
        fr.y, fr.u, fr.v = (p.to(device, non_blocking=non_blocking) for p in self.planes())
        return fr

    def cpu(self):
        return self.to('cpu')

    def to_semiplanar(self):
        """The same codes as a YuvSpFrame (depth 10 | 12, '420' | '422'): word = code << (16 - depth), U and V interleaved.  Plain torch ops
        on the frame's device: a copy."""
        check_layout('semiplanar', self.depth, self.subsampling)
        mask, sh = (1 << self.depth) - 1, 16 - self.depth
        word = lambda p: ((p.to(torch.int32) & mask) << sh).to(torch.int16)
        return YuvSpFrame(word(self.y), torch.stack([word(self.u), word(self.v)], -1).flatten(1), self.depth, self.subsampling)


def frame_bytes2(width, height, subsampling='420', depth=8):
    return FrameFormat('planar', depth, subsampling).frame_bytes(width, height)


def read_yuv(path, width, height, subsampling='420', depth=8, frames=None, start=0):
    """A raw planar .yuv file of `width` x `height` frames (yuv420p, yuv422p10le, yuv444p12le ...) -> list of YuvFrame on the CPU (all of
    them, or the first `frames`; from frame `start` on).  As read_yuv420: ONE buffer, pinned when a GPU is there, the planes views of it.  ValueError: sides that do
    not fit the subsampling, a file size that is not a whole number of frames, an unknown depth / subsampling, a code beyond the depth."""
    _check2(depth, subsampling)
    return FrameFormat('planar', depth, subsampling).read(path, width, height, frames, start, 'read_yuv')


# ----------------------------------------------------------------------------------------------- semi-planar 10 / 12 bits: P010 and kin
SP_DEPTHS, SP_SUBSAMPLINGS = (10, 12), ('420', '422')
SP_LAYOUTS = {'p010': (10, '420'), 'p012': (12, '420'), 'p210': (10, '422'), 'p212': (12, '422')}       # name -> (depth, subsampling)


class YuvSpFrame:
    """One semi-planar frame of `depth` 10 | 12 bits at `subsampling` '420' | '422' (P010 / P012 / P210 / P212): a luma plane y (h, w) and a
    chroma plane uv of (h/2 | h, w/2) chroma pixels, each two neighbouring words U, V -- given as (ch, 2 cw) or (ch, cw, 2) and kept as
    (ch, 2 cw) -- torch.int16 on one device: the 16 bits of the container with the value in the HIGH bits, code = word >> (16 - depth).
    The low bits are ignored, whatever they hold.  numpy uint16 arrays are reinterpreted, not copied.  w is even, and h for 4:2:0."""

    def __init__(self, y, uv, depth=10, subsampling='420'):
        check_layout('semiplanar', depth, subsampling)

        def t(a):
            if isinstance(a, torch.Tensor):
                return a
            a = np.asarray(a)
            return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
        y, uv = t(y), t(uv)
        if y.dim() != 2 or y.dtype != torch.int16:
            raise ValueError(f'y is an (h, w) torch.int16 plane, got {tuple(y.shape)} {y.dtype}')
        h, w = int(y.shape[0]), int(y.shape[1])
        if not _extent_ok(h, w, subsampling):
            raise ValueError(f'a {subsampling} frame has positive sides, even where the chroma is subsampled, got {h} x {w}')
        ch = h >> SHIFTS[subsampling][1]
        if uv.dtype != torch.int16 or tuple(uv.shape) not in ((ch, w), (ch, w // 2, 2)) or uv.device != y.device:
            raise ValueError(f'uv is a ({ch}, {w}) or ({ch}, {w // 2}, 2) torch.int16 plane on the device of y, got {tuple(uv.shape)} {uv.dtype}')
        self.y, self.uv, self.depth, self.subsampling, self.h, self.w = y, uv.flatten(1) if uv.dim() == 3 else uv, depth, subsampling, h, w

    @property
    def device(self):
        return self.y.device

    @property
    def size(self):
        return (self.h, self.w)

    def planes(self):
        """The planes in file order: (y, uv)."""
        return (self.y, self.uv)

    def to(self, device, non_blocking=False):
        if torch.device(device) == self.device:
            return self
        return YuvSpFrame(self.y.to(device, non_blocking=non_blocking), self.uv.to(device, non_blocking=non_blocking), self.depth, self.subsampling)

    def cpu(self):
        return self.to('cpu')

    def to_planar(self):
        """The same codes as a YuvFrame: code = word >> (16 - depth) (the word read as unsigned), U and V deinterleaved.  Plain torch ops on
        the frame's device: a copy."""
        sh = 16 - self.depth
        code = lambda p: ((p.to(torch.int32) & 0xffff) >> sh).to(torch.int16)
        uv = self.uv.unflatten(1, (self.w // 2, 2))
        return YuvFrame(code(self.y), code(uv[..., 0]), code(uv[..., 1]), self.depth, self.subsampling)


def read_yuv_sp(path, width, height, depth=10, subsampling='420', frames=None, start=0):
    """A raw P010 / P012 / P210 / P212 file of `width` x `height` frames (per frame the Y plane, then the UV plane, little-endian words) ->
    list of YuvSpFrame on the CPU (all of them, or the first `frames`; from frame `start` on).  As read_yuv: ONE buffer, pinned when a GPU is there, the planes
    views of it.  ValueError: sides that do not fit, a file size that is not a whole number of frames, an unsupported depth / subsampling."""
    if depth not in SP_DEPTHS or subsampling not in SP_SUBSAMPLINGS:
        raise ValueError(f'read_yuv_sp: semi-planar frames are {SP_DEPTHS} bits at {SP_SUBSAMPLINGS}, got {depth!r} bits at {subsampling!r}')
    return FrameFormat('semiplanar', depth, subsampling).read(path, width, height, frames, start, 'read_yuv_sp')


# ----------------------------------------------------------------------------------------------- one description of a frame's format
class FrameFormat(namedtuple('FrameFormat', 'layout depth subsampling')):
    """What the three frame classes differ in, as one immutable value: `layout` 'planar' (YuvFrame), 'semiplanar' (YuvSpFrame), 'i420' /
    'nv12' (Yuv420Frame), `depth` and `subsampling`.  ValueError for a combination that does not exist (utils.yuvseq.check_layout; `siting`
    and `matrix` are checked with it where the caller has them, not kept).  Whatever depends on the kind of a frame -- its bytes in a file,
    reading, allocating, cropping, batching -- is a method here, so that no caller branches on a frame's class."""
    __slots__ = ()

    def __new__(cls, layout='planar', depth=8, subsampling='420', siting='center', matrix='bt709'):
        check_layout(layout, depth, subsampling, siting, matrix)
        return super().__new__(cls, layout, depth, subsampling)

    @classmethod
    def of(cls, frame):
        """The format of a frame (not checked again: the frame's class did that when the frame was made)."""
        if isinstance(frame, Yuv420Frame):
            return cls._make((frame.fmt, 8, '420'))
        if isinstance(frame, (YuvFrame, YuvSpFrame)):
            return cls._make(('semiplanar' if isinstance(frame, YuvSpFrame) else 'planar', frame.depth, frame.subsampling))
        raise ValueError(f'expected a frame of utils.yuv, got {type(frame).__name__}')

    @classmethod
    def shared(cls, frames, who):
        """(list(frames), the format of the first).  ValueError: no frames, something that is not a frame, kinds, depths or subsamplings
        mixed in one call.  I420 and NV12 frames may meet in a list: the host expressions take both, and a launch refuses them itself."""
        fs = list(frames)
        if not fs:
            raise ValueError(f'{who}: no frames')
        fmts = [cls.of(f) for f in fs]
        if any(f != fmts[0] and not (f.layout in FORMATS and fmts[0].layout in FORMATS) for f in fmts):
            raise ValueError(f'{who}: frames of different kinds, depths or subsamplings may not be mixed in one call, got '
                             f'{sorted(set(map(tuple, fmts)))}')
        return fs, fmts[0]

    @property
    def dtype(self):
        return torch.uint8 if self.depth == 8 else torch.int16

    @property
    def interleaved(self):
        """One chroma plane of (U, V) pairs behind y, not a u and a v plane."""
        return self.layout in ('semiplanar', 'nv12')

    def _chroma_shapes(self, h, w):
        sx, sy = SHIFTS[self.subsampling]
        return ((h >> sy, w >> sx, 2),) if self.interleaved else ((h >> sy, w >> sx),) * 2

    def frame(self, y, *chroma, scan=True):
        """The frame of this format on planes given in file order: (y, u, v) or (y, uv)."""
        if self.layout == 'i420':
            return Yuv420Frame('i420', y, *chroma)
        if self.layout == 'nv12':
            return Yuv420Frame('nv12', y, uv=chroma[0])
        if self.layout == 'semiplanar':
            return YuvSpFrame(y, chroma[0], self.depth, self.subsampling)
        return YuvFrame(y, *chroma, self.depth, self.subsampling, scan=scan)

    def frame_bytes(self, width, height):
        """The bytes of one frame in a raw file; a semi-planar frame holds as many samples as the planar one."""
        sx, sy = SHIFTS[self.subsampling]
        return (width * height + 2 * (width >> sx) * (height >> sy)) * (1 if self.depth == 8 else 2)

    def read(self, path, width, height, frames=None, start=0, who='FrameFormat.read'):
        """A raw file of `width` x `height` frames of this format -> list of frames on the CPU (all of them, or the first `frames`; from
        frame `start` on).  The file is read into ONE buffer -- pinned when a GPU is there, so a frame's upload is an asynchronous copy
        -- and the planes are views of it.  ValueError: sides that do not fit the subsampling, a file size that is not a whole number of
        frames, a planar code beyond the depth."""
        if not _extent_ok(height, width, self.subsampling):
            raise ValueError(f'{who}: {width} x {height} does not fit subsampling {self.subsampling}')
        shapes = ((height, width),) + self._chroma_shapes(height, width)
        counts = [math.prod(s) for s in shapes]
        return [self.frame(*(p.view(s) for p, s in zip(fr.view(self.dtype).split(counts), shapes)))
                for fr in _read_raw(path, self.frame_bytes(width, height), frames, start, who)]

    def new(self, h, w, device):
        """An uninitialised (h, w) frame of this format on `device`."""
        empty = lambda s: torch.empty(s, dtype=self.dtype, device=device)
        return self.frame(empty((h, w)), *(empty(s) for s in self._chroma_shapes(h, w)), scan=False)

    def crop(self, frame, y, x, th, tw):
        """The window (y, x, th, tw) of a frame of this format -- on the chroma grid -- as a frame whose planes are views of the frame's."""
        sx, sy = SHIFTS[self.subsampling]
        rows = slice(y >> sy, (y + th) >> sy)
        # a semi-planar UV row holds w samples: chroma pixel x / 2 starts at sample x (the uv of NV12 is indexed by chroma pixel, as u and v)
        cols = slice(x, x + tw) if self.layout == 'semiplanar' else slice(x >> sx, (x + tw) >> sx)
        return self.frame(frame.y[y:y + th, x:x + tw], *(p[rows, cols] for p in frame.planes()[1:]), scan=False)

    def batch(self, frames, div, device, matrix='bt709', range='limited', chroma='bilinear', siting='center', coded=None, filter='lanczos3'):
        """The _Batch of frames of this format that the codecs hand to compress_batch: Yuv420Batch (which takes no siting: ValueError
        unless it is 'center'), YuvBatch or YuvSpBatch.  coded = (h, w): a ScaledYuvBatch instead, whose `fill` resamples the frames
        (of ONE size) to that size with `filter` on the way."""
        check_layout(*self, siting, matrix)
        if coded is not None:
            return ScaledYuvBatch(self, frames, coded, filter, div, device, matrix, range, chroma, siting)
        if self.layout in FORMATS:
            return Yuv420Batch(frames, div, device, matrix, range, chroma)
        return (YuvSpBatch if self.layout == 'semiplanar' else YuvBatch)(frames, div, device, matrix, range, chroma, siting)


def write_frames(frames, path, append=False):
    """Write frames of any kind (any device) to a raw file, each in its own plane layout, one after the other; 16-bit samples
    little-endian."""
    with open(path, 'ab' if append else 'wb') as f:
        for fr in frames:
            for p in fr.planes():
                a = p.cpu().contiguous().numpy()
                f.write((a if a.dtype == np.uint8 else a.astype('<i2', copy=False)).tobytes())


write_yuv420 = write_yuv = write_yuv_sp = write_frames


# ----------------------------------------------------------------------------------------------- the defining expressions (CPU, fp32)
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _scales2(depth, range):
    """fp32 luma offset, luma scale, chroma offset, chroma scale and the largest code (all integers: exact)."""
    s, peak = float(1 << (depth - 8)), float((1 << depth) - 1)
    vals = (16.0 * s, 219.0 * s, 128.0 * s, 224.0 * s) if range == 'limited' else (0.0, peak, 128.0 * s, peak)
    return tuple(_f32(k) for k in vals) + (peak,)


def _codes_f32(p, depth):
    """A plane's codes as fp32 (exact); 16-bit containers are masked to `depth` bits, as the kernels do."""
    return p.to(torch.float32) if p.dtype == torch.uint8 else (p.to(torch.int32) & ((1 << depth) - 1)).to(torch.float32)


def _upsample_axis(c, dim, chroma, left):
    """fp32 chroma, one subsampled axis doubled.  'nearest': sample x >> 1.  'bilinear', centre: 3/4 of the sample a pixel lies in and 1/4 of
    the neighbour on the pixel's side; left: position 2k takes sample k, position 2k + 1 takes (c[k] + c[k + 1]) / 2.  Indices are clamped
    at the plane's edges; the weights are dyadic and the codes small integers: exact in fp32."""
    if chroma == 'nearest':
        return c.repeat_interleave(2, dim)
    n = c.shape[dim]
    i = torch.arange(n)
    nxt = c.index_select(dim, (i + 1).clamp(max=n - 1))
    if left:
        even, odd = c, (c + nxt) * 0.5
    else:
        prev = c.index_select(dim, (i - 1).clamp(min=0))
        even, odd = c * 0.75 + prev * 0.25, c * 0.75 + nxt * 0.25
    return torch.stack([even, odd], dim + 1).flatten(dim, dim + 1)


def _upsample2(c, depth, subsampling, siting, chroma):
    sx, sy = SHIFTS[subsampling]
    c = _codes_f32(c, depth)
    if sy:
        c = _upsample_axis(c, 0, chroma, False)              # vertically the chroma is centred for both sitings
    if sx:
        c = _upsample_axis(c, 1, chroma, siting == 'left')
    return c


def yuv_to_rgb_expr2(y, u, v, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', chroma='bilinear'):
    """THE DEFINITION of lvae_image_yuv_to_f32 inside a frame's extent: the planes of a YuvFrame on the CPU -> (3, h, w) fp32 RGB in
    [0, 1]."""
    _check2(depth, subsampling, siting, matrix, range, chroma)
    _, _, _, a, b, d, e = (_f32(k) for k in COEF[matrix])
    yo, ys, co, cs, _ = _scales2(depth, range)
    yn = (_codes_f32(y, depth) - yo) / ys
    cb = (_upsample2(u, depth, subsampling, siting, chroma) - co) / cs
    cr = (_upsample2(v, depth, subsampling, siting, chroma) - co) / cs
    r = yn + a * cr
    bl = yn + b * cb
    g = (yn - d * cb) - e * cr
    return torch.stack([r, g, bl]).clamp(0, 1)


def _downsample2(c, subsampling, siting):
    """Per-pixel fp32 colour differences (h, w) -> the chroma plane's; the order of the sums is part of the definition."""
    sx, sy = SHIFTS[subsampling]
    if not sx:
        return c
    if siting == 'left':
        k = torch.arange(c.shape[1] // 2)
        prev = c.index_select(1, (2 * k - 1).clamp(min=0))
        h = ((prev + c[:, 1::2]) + (c[:, 0::2] + c[:, 0::2])) * 0.25
        return (h[0::2] + h[1::2]) * 0.5 if sy else h
    if sy:
        return ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * 0.25
    return (c[:, 0::2] + c[:, 1::2]) * 0.5


def rgb_to_yuv_expr2(x, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited'):
    """THE DEFINITION of lvae_image_f32_to_yuv: (3, h, w) fp32 RGB on the CPU (sides that fit the subsampling) -> planes y, u, v of codes
    (uint8 at depth 8, int16 above).  Values are clamped to [0, 1] first and a NaN counts as 0; codes are rint (ties to even) of
    value * scale + offset, clamped to 0 .. 2^depth - 1."""
    _check2(depth, subsampling, siting, matrix, range)
    kr, kg, kb, a, b, _, _ = (_f32(k) for k in COEF[matrix])
    yo, ys, co, cs, peak = _scales2(depth, range)
    x = x.to(torch.float32)
    x = torch.where(x > 0, x, torch.zeros((), dtype=torch.float32))
    x = torch.where(x < 1, x, torch.ones((), dtype=torch.float32))
    r, g, bl = x[0], x[1], x[2]
    yn = (kr * r + kg * g) + kb * bl
    cb, cr = (bl - yn) / b, (r - yn) / a
    code = lambda t: torch.round(t).clamp(0, peak).to(torch.uint8 if depth == 8 else torch.int16)
    return (code(yn * ys + yo), code(_downsample2(cb, subsampling, siting) * cs + co), code(_downsample2(cr, subsampling, siting) * cs + co))


def yuv_to_rgb_expr(y, u, v, matrix='bt709', range='limited', chroma='bilinear'):
    """THE DEFINITION of lvae_image_yuv420_to_f32 inside a frame's extent: uint8 planes y (h, w), u, v (h/2, w/2) on the CPU -> (3, h, w)
    fp32 RGB in [0, 1]: yuv_to_rgb_expr2 at depth 8, '420', 'center', for BT.601 / BT.709."""
    _check(matrix, range, chroma)
    return yuv_to_rgb_expr2(y, u, v, 8, '420', 'center', matrix, range, chroma)


def rgb_to_yuv_expr(x, matrix='bt709', range='limited'):
    """THE DEFINITION of lvae_image_f32_to_yuv420: (3, h, w) fp32 RGB on the CPU, h and w even -> uint8 planes y (h, w), u, v (h/2, w/2):
    rgb_to_yuv_expr2 at depth 8, '420', 'center', for BT.601 / BT.709.  Values are clamped to [0, 1] first and a NaN counts as 0."""
    _check(matrix, range)
    return rgb_to_yuv_expr2(x, 8, '420', 'center', matrix, range)


# ----------------------------------------------------------------------------------------------- batches and the kernel path
def _as_frames(frames, frame_type):
    fs = list(frames)
    for f in fs:
        if not isinstance(f, frame_type):
            raise ValueError(f'expected a {frame_type.__name__}, got {type(f).__name__}')
    if not fs:
        raise ValueError('no frames')
    return fs


def _share_layout(fs):
    if any((f.depth, f.subsampling) != (fs[0].depth, fs[0].subsampling) for f in fs):
        raise ValueError('the frames of one call share depth and subsampling')


def _plane_args(frames, names):
    """Host arrays, as the native entries take them, of device frames' planes `names` (None: an argument the entry does not read):
    addresses, row strides in samples, the (h, w) pairs -- and, last, what had to be made contiguous, to be kept alive."""
    n = len(frames)
    # a plane is read where it lies if its rows are dense -- (h, w), or (h, w / 2, 2) for the uv of NV12 -- and do not overlap
    # (strides and sizes only: indexing a tensor here costs more host time than the launch)
    rows_ok = lambda p: p.stride(-1) == 1 and (p.dim() == 2 or p.stride(1) == 2) and p.stride(0) >= p.size(1) * (p.dim() - 1)
    ps = [k and [p if rows_ok(p) else p.contiguous() for p in (getattr(f, k) for f in frames)] for k in names]
    ptrs = [q and (ctypes.c_void_p * n)(*[p.data_ptr() for p in q]) for q in ps]
    rows = [q and (ctypes.c_long * n)(*[p.stride(0) for p in q]) for q in ps]
    hw = (ctypes.c_int * (2 * n))(*[v for f in frames for v in f.size])
    return ptrs, rows, hw, ps


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Batch:
    """B frames on one device that share a canvas (H, W) >= their own sizes, with the parameters of their conversion: the
    utils.image.U8Batch counterpart that the codecs hand to compress_batch as `u8=`.  `shape` is the fp32 tensor's; `fill(dst, start, n)`
    converts frames start .. start + n straight into `dst` -- an (n, 3, H, W) fp32 view of an encode plan's input -- with one launch on
    the current stream.  A subclass's `_entry(frames)` says which entry that is: its name, the planes it takes and the codes before `dst`."""

    def __init__(self, fs, div, device):
        self.sizes = [f.size for f in fs]
        H, W = _canvas(self.sizes, div)
        self.shape = (len(fs), 3, H, W)
        self.device = torch.device(device)
        self.frames = [f.to(self.device, non_blocking=True) for f in fs]      # the file's bytes cross the bus, unpadded

    def fill(self, dst, start=0, n=None):
        from .. import _native
        n = len(self.frames) - start if n is None else n
        _, _, H, W = self.shape
        assert dst.dtype == torch.float32 and dst.device == self.device and tuple(dst.shape) == (n, 3, H, W) and dst[0].is_contiguous()
        entry, names, codes = self._entry(self.frames[start:start + n])
        ptrs, rows, hw, keep = _plane_args(self.frames[start:start + n], names)
        with torch.cuda.device(self.device):
            _native.check(getattr(_native.lib(), 'lvae_' + entry)(*ptrs, *rows, hw, n, *codes, CHROMA.index(self.chroma), dst.data_ptr(),
                                                                 dst.stride(0) if n > 1 else 3 * H * W, H, W, _stream(self.device)), entry)
        del keep


def _fmt_names(frames):
    """The planes of Yuv420Frames of ONE format as lvae_image_yuv420_to_f32 / lvae_image_f32_to_yuv420 take them: NV12 has no v."""
    if any(f.fmt != frames[0].fmt for f in frames):
        raise ValueError('the frames of one call share a plane layout (use Yuv420Frame.as_format)')
    return ('y', 'u', 'v') if frames[0].fmt == 'i420' else ('y', 'uv', None)


class Yuv420Batch(_Batch):
    """_Batch of Yuv420Frames: what CodecBase.compress_yuv420 hands to compress_batch; 1.5 bytes per pixel cross the bus."""

    def __init__(self, frames, div, device, matrix='bt709', range='limited', chroma='bilinear'):
        _check(matrix, range, chroma)
        self.matrix, self.range, self.chroma = matrix, range, chroma
        super().__init__(_as_frames(frames, Yuv420Frame), div, device)

    def _entry(self, frames):
        return 'image_yuv420_to_f32', _fmt_names(frames), (FORMATS.index(frames[0].fmt), MATRICES.index(self.matrix), RANGES.index(self.range))


class YuvBatch(_Batch):
    """_Batch of YuvFrames of one depth and subsampling: what CodecBase.compress_yuv hands to compress_batch."""

    frame_type, entry, names = YuvFrame, 'image_yuv_to_f32', ('y', 'u', 'v')

    def __init__(self, frames, div, device, matrix='bt709', range='limited', chroma='bilinear', siting='center'):
        fs = _as_frames(frames, self.frame_type)
        self.depth, self.subsampling = fs[0].depth, fs[0].subsampling
        _share_layout(fs)
        _check2(self.depth, self.subsampling, siting, matrix, range, chroma)
        self.matrix, self.range, self.chroma, self.siting = matrix, range, chroma, siting
        super().__init__(fs, div, device)

    def _entry(self, frames):
        return self.entry, self.names, (self.depth, SUBSAMPLINGS.index(self.subsampling), SITINGS.index(self.siting),
                                        MATRICES2.index(self.matrix), RANGES.index(self.range))


class YuvSpBatch(YuvBatch):
    """YuvBatch for YuvSpFrames: the two planes of every frame go to the device as the file holds them, and `fill` is one
    lvae_image_yuvsp_to_f32 launch -- no deinterleaved or shifted copy exists anywhere."""
    frame_type, entry, names = YuvSpFrame, 'image_yuvsp_to_f32', ('y', 'uv')


def _to_rgb(fs, div, device, expr, batch):
    """The two paths of to_rgb01 / to_rgb01_any.  CPU frames with device=None: expr(frame), replicate-padded to the canvas and stacked.
    Otherwise batch(device) filled into a new tensor on `device` (default: the first frame's that is not the CPU)."""
    if device is None and all(f.device.type == 'cpu' for f in fs):
        sizes = [f.size for f in fs]
        H, W = _canvas(sizes, div)
        out = []
        for f in fs:
            x = expr(f)
            out.append(F.pad(x.unsqueeze(0), (0, W - f.w, 0, H - f.h), mode='replicate')[0] if f.size != (H, W) else x)
        return torch.stack(out), sizes
    b = batch(next(f.device for f in fs if f.device.type != 'cpu') if device is None else device)
    out = torch.empty(b.shape, dtype=torch.float32, device=b.device)
    b.fill(out)
    return out, b.sizes


def to_rgb01(frames, div=1, device=None, matrix='bt709', range='limited', chroma='bilinear'):
    """A list of Yuv420Frame -> ((B, 3, H, W) fp32 RGB in [0, 1], [(h, w)]): chroma upsampled ('nearest' | 'bilinear', centre siting),
    the inverse matrix applied, clamped, every frame replicate-padded on the right / bottom to the common canvas, the smallest (H, W) of
    multiples of `div` that holds them all.  CPU frames with device=None: the defining expression on the host.  Otherwise: one upload
    of each frame's bytes (none for device frames) and one kernel launch for the batch, on `device` (default: the frames' device)."""
    fs = _as_frames(frames, Yuv420Frame)
    _check(matrix, range, chroma)
    return to_rgb01_any(fs, div, device, matrix, range, chroma)


def to_rgb01_any(frames, div=1, device=None, matrix='bt709', range='limited', chroma='bilinear', siting='center'):
    """to_rgb01 for a list of YuvFrame of one depth and subsampling -> ((B, 3, H, W) fp32 RGB in [0, 1], [(h, w)]).  siting: 'center' |
    'left' (where the chroma samples lie horizontally; see the module docstring); matrix also 'bt2020'.  CPU frames with device=None: the
    defining expression on the host.  Otherwise one upload of each frame's bytes and one kernel launch for the batch.  A list of
    YuvSpFrame is taken too: on the host through to_planar (the definition), on the device by its own kernel.  So is a list of
    Yuv420Frame, which has siting 'center' and no 'bt2020': the call to_rgb01 makes."""
    fs, fmt = FrameFormat.shared(frames, 'to_rgb01_any')
    check_layout(*fmt, siting, matrix)
    _check2(range=range, chroma=chroma)

    def expr(f):
        p = f.to_planar() if fmt.layout == 'semiplanar' else f
        return yuv_to_rgb_expr2(p.y, p.u, p.v, fmt.depth, fmt.subsampling, siting, matrix, range, chroma)
    return _to_rgb(fs, div, device, expr, lambda dev: fmt.batch(fs, div, dev, matrix, range, chroma, siting))


def _rgb_items(x, sizes, who):
    """The prelude of from_rgb01 / from_rgb01_any: x as a list of (3, h, w) views cut to `sizes`."""
    from .views import items
    xs = items(x, 'x')
    if sizes is not None:
        if len(sizes) != len(xs):
            raise ValueError(f'{who}: {len(sizes)} sizes for {len(xs)} images')
        xs = [v[:, :h, :w] for v, (h, w) in zip(xs, sizes)]
    if not xs or any(v.shape[0] != 3 or v.shape[1] == 0 or v.shape[2] == 0 for v in xs):
        raise ValueError(f'{who}: expected 3-channel, non-empty images')
    return xs


def _from_rgb(xs, outs, names, entry, codes):
    """Device images xs -> the planes `names` of the frames `outs` (of the images' sizes), by one launch of `entry` on the current stream."""
    from .. import _native
    from .views import strided_batch
    B, device = len(xs), xs[0].device
    hmax, wmax = max(f.h for f in outs), max(f.w for f in outs)
    with torch.cuda.device(device):
        keep, px, (s_img, s_plane, s_row) = strided_batch(xs, hmax, wmax, device)
        span = (hmax - 1) * s_row + wmax             # views whose common strides do not hold the largest extent are packed instead
        if s_row < wmax or s_plane < span or (B > 1 and s_img < 2 * s_plane + span):
            keep, px, (s_img, s_plane, s_row) = strided_batch([v.clone() for v in xs], hmax, wmax, device)
        ptrs, rows, hw, _ = _plane_args(outs, names)
        _native.check(getattr(_native.lib(), 'lvae_' + entry)(px, s_img if B > 1 else 3 * s_plane, s_plane, s_row, hmax, wmax, hw, B, *codes,
                                                             *ptrs, *rows, _stream(device)), entry)
    del keep
    return outs


def from_rgb01(x, sizes=None, fmt='i420', matrix='bt709', range='limited'):
    """The inverse: fp32 RGB images in [0, 1] -> a list of Yuv420Frame of layout `fmt` on the same device.  Values are clamped to [0, 1]
    (NaN -> 0), the forward matrix is applied per pixel, a chroma sample is the mean of its 2x2 block, bytes are rounded with ties to
    even.  x: a (B, 3, H, W) tensor or a list of (1, 3, h, w) / (3, h, w) tensors (crops of a decoder's padded batch are read in place);
    sizes: per-image valid extents [(h, w)] (default: every item whole); odd extents raise ValueError.  Device tensors: one kernel launch
    for the batch on the current stream; CPU tensors: the defining expression."""
    _check(matrix, range, fmt=fmt)
    xs = _rgb_items(x, sizes, 'from_rgb01')
    if any(v.shape[1] % 2 or v.shape[2] % 2 for v in xs):
        raise ValueError(f'from_rgb01: a 4:2:0 frame has even sides, got {[tuple(v.shape[1:]) for v in xs]}')
    return from_rgb01_any(xs, matrix=matrix, range=range, layout=fmt)


def from_rgb01_any(x, sizes=None, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited', layout='planar'):
    """from_rgb01 for YuvFrames: fp32 RGB images in [0, 1] -> a list of YuvFrame of `depth` and `subsampling` on the same device, the
    chroma sampled for `siting`.  x, sizes: as in from_rgb01; extents that do not fit the subsampling raise ValueError.  Device tensors: one
    kernel launch for the batch on the current stream; CPU tensors: the defining expression.  layout 'semiplanar' (depth 10 | 12, '420' |
    '422'): a list of YuvSpFrame holding the same codes, written by lvae_image_f32_to_yuvsp (CPU: to_semiplanar of the expression's frame).
    layout 'i420' / 'nv12' (depth 8, '420', 'center', 'bt601' | 'bt709'): a list of Yuv420Frame, written by lvae_image_f32_to_yuv420 -- the
    call from_rgb01 makes.  ValueError: a layout that these parameters do not have (utils.yuvseq.check_layout)."""
    _check2(range=range)
    fmt = FrameFormat(layout, depth, subsampling, siting, matrix)
    xs = _rgb_items(x, sizes, 'from_rgb01_any')
    hw = [(int(v.shape[1]), int(v.shape[2])) for v in xs]
    if any(not _extent_ok(h, w, subsampling) for h, w in hw):
        raise ValueError(f'from_rgb01_any: sizes {hw} do not fit subsampling {subsampling}')
    device, sp = xs[0].device, layout == 'semiplanar'
    if device.type == 'cpu':
        planes = [rgb_to_yuv_expr2(v, depth, subsampling, siting, matrix, range) for v in xs]
        if layout in FORMATS:
            return [Yuv420Frame('i420', *p).as_format(layout) for p in planes]
        outs = [YuvFrame(*p, depth, subsampling) for p in planes]
        return [f.to_semiplanar() for f in outs] if sp else outs
    outs = [fmt.new(h, w, device) for h, w in hw]
    if layout in FORMATS:
        return _from_rgb(xs, outs, _fmt_names(outs), 'image_f32_to_yuv420', (FORMATS.index(layout), MATRICES.index(matrix), RANGES.index(range)))
    codes = (depth, SUBSAMPLINGS.index(subsampling), SITINGS.index(siting), MATRICES2.index(matrix), RANGES.index(range))
    return _from_rgb(xs, outs, (YuvSpBatch if sp else YuvBatch).names, 'image_f32_to_yuvsp' if sp else 'image_f32_to_yuv', codes)


# ----------------------------------------------------------------------------------------------- frames at reduced resolution
# csrc/resample_yuv.hip: the resampler of utils/resample.py fused with the two conversions above.  The DEFINITION is the composition in
# the RGB domain -- resize(to_rgb01_any(frames), size, clamp=True) on the way in, from_rgb01_any(resize(x, size)) on the way out -- and the
# kernels give its bits without the full-resolution fp32 image it puts into memory.
_XSPANS = {}


def _scaled_tables(src, dst, filter, device):
    """The table arguments of lvae_resample_yuv_to_f32 / lvae_resample_f32_to_yuv for (h, w) src -> dst: the seven of lvae_resample_*, then
    `xspan`, the largest number of source columns 8 consecutive output columns read (0 for an axis that keeps its size)."""
    from . import resample
    from .image import _tables
    tabs = _tables(*src, *dst, filter, device)
    key = (int(src[1]), int(dst[1]), filter)
    if key not in _XSPANS:
        start, wgt = resample.axis_table(*key)
        _XSPANS[key] = 0 if key[0] == key[1] else resample.tile_span(start, wgt.shape[1], key[0], rows=8)
    return tabs, _XSPANS[key]


def _kind_codes(fmt, siting, matrix, range):
    """depth, subsampling, siting, matrix, range as the native entries take them, and the names of a frame's planes with its layout code."""
    codes = (fmt.depth, SUBSAMPLINGS.index(fmt.subsampling), SITINGS.index(siting), MATRICES2.index(matrix), RANGES.index(range))
    return codes, (('y', 'uv', None) if fmt.interleaved else ('y', 'u', 'v')), LAYOUTS.index('semiplanar' if fmt.interleaved else 'planar')


def _one_kind(fs, who):
    fmt, size = FrameFormat.of(fs[0]), fs[0].size
    if any(FrameFormat.of(f) != fmt or f.size != size for f in fs):
        raise ValueError(f'{who}: the frames of one scaled call share one kind, one plane layout and one size')
    return size


class ScaledYuvBatch(_Batch):
    """B frames of ONE kind and size on one device, coded at `coded` = (h, w): what CodecBase.compress_yuv_scaled hands to compress_batch
    as `u8=`, the utils.image.ScaledU8Batch of YUV frames.  `sizes` are the coded sizes (what the models' containers record), `shape` the
    coded canvas; `fill` converts and resamples frames start .. start + n straight into an encode plan's input -- `filter`, clamped to
    [0, 1], replicate-padded -- with one launch (lvae_resample_yuv_to_f32).  With coded == the frames' size that is the plain
    conversion's result, bit for bit.  canvas: the (H, W) of `shape` instead of the coded size rounded up to multiples of `div`."""

    def __init__(self, fmt, frames, coded, filter, div, device, matrix='bt709', range='limited', chroma='bilinear', siting='center', canvas=None):
        from . import resample
        fs = list(frames)
        check_layout(*fmt, siting, matrix)
        _check2(range=range, chroma=chroma)
        resample._filter(filter)
        if not fs:
            raise ValueError('no frames')
        self.src_size = _one_kind(fs, 'ScaledYuvBatch')
        if FrameFormat.of(fs[0]) != fmt:
            raise ValueError(f'ScaledYuvBatch: the frames are {tuple(FrameFormat.of(fs[0]))}, not {tuple(fmt)}')
        coded = (int(coded[0]), int(coded[1]))
        resample.check_ratio(self.src_size[0], coded[0])
        resample.check_ratio(self.src_size[1], coded[1])
        super().__init__(fs, 1, device)
        self.fmt, self.filter, self.matrix, self.range, self.chroma, self.siting = fmt, filter, matrix, range, chroma, siting
        self.sizes = [coded] * len(fs)
        self.shape = (len(fs), 3) + (_canvas(self.sizes, div) if canvas is None else (int(canvas[0]), int(canvas[1])))
        if self.shape[2] < coded[0] or self.shape[3] < coded[1]:
            raise ValueError(f'ScaledYuvBatch: canvas {self.shape[2:]} is below the coded size {coded}')
        self._tabs, self._xspan = _scaled_tables(self.src_size, coded, filter, self.device)

    def fill(self, dst, start=0, n=None):
        from .. import _native
        n = len(self.frames) - start if n is None else n
        _, _, H, W = self.shape
        assert dst.dtype == torch.float32 and dst.device == self.device and tuple(dst.shape) == (n, 3, H, W) and dst[0].is_contiguous()
        codes, names, layout = _kind_codes(self.fmt, self.siting, self.matrix, self.range)
        ptrs, rows, hw, keep = _plane_args(self.frames[start:start + n], names)
        with torch.cuda.device(self.device):
            _native.check(_native.lib().lvae_resample_yuv_to_f32(*ptrs, *rows, hw, n, *codes, CHROMA.index(self.chroma), layout, *self.src_size,
                                                                 *self.sizes[0], *self._tabs, self._xspan, dst.data_ptr(),
                                                                 dst.stride(0) if n > 1 else 3 * H * W, H, W, _stream(self.device)),
                          'resample_yuv_to_f32')
        del keep


def to_rgb01_scaled(frames, size, filter='lanczos3', canvas=None, matrix='bt709', range='limited', chroma='bilinear', siting='center',
                    device=None):
    """Frames of ONE kind and size (anything to_rgb01_any takes) -> a (B, 3, H, W) fp32 tensor: every frame converted to RGB in [0, 1]
    and resized to size = (h, w) with the resampler of utils/resample.py (`filter`), clamped to [0, 1] and replicate-padded to
    canvas = (H, W) >= size (default: size).  The definition is utils.image.resize(to_rgb01_any(frames)[0], size, filter, clamp=True).
    Frames on a GPU (or `device`): one launch of lvae_resample_yuv_to_f32 per 16 frames gives those bits, and no full-resolution RGB
    image is made.  CPU frames with device=None take the composition of the two CPU paths (the defining expression of the conversion,
    then resample.resize_reference, fp64 cast to fp32).  ValueError: frames of different kinds or sizes, an unknown filter, a ratio
    outside [1/8, 8] on an axis, a canvas below size."""
    from .image import resize
    fs, fmt = FrameFormat.shared(frames, 'to_rgb01_scaled')
    _one_kind(fs, 'to_rgb01_scaled')
    size = (int(size[0]), int(size[1]))
    H, W = size if canvas is None else (int(canvas[0]), int(canvas[1]))
    if H < size[0] or W < size[1]:
        raise ValueError(f'to_rgb01_scaled: canvas {(H, W)} is below size {size}')
    if device is None and all(f.device.type == 'cpu' for f in fs):
        x = resize(to_rgb01_any(fs, 1, None, matrix, range, chroma, siting)[0], size, filter, clamp=True)
        return F.pad(x, (0, W - size[1], 0, H - size[0]), mode='replicate') if (H, W) != size else x
    device = next(f.device for f in fs if f.device.type != 'cpu') if device is None else device
    b = ScaledYuvBatch(fmt, fs, size, filter, 1, device, matrix, range, chroma, siting, canvas=(H, W))
    out = torch.empty(b.shape, dtype=torch.float32, device=b.device)
    b.fill(out)
    return out


def from_rgb01_scaled(xs, size, filter='lanczos3', depth=8, subsampling='420', siting='center', matrix='bt709', range='limited',
                      layout='planar', outs=None):
    """The way out: fp32 RGB images of ONE size -- a (B, 3, h, w) tensor or a list of (1, 3, h, w) / (3, h, w) views (crops of a decoder's
    padded batch are read in place) -> a list of frames of size = (h, w) on the same device, of the kind from_rgb01_any's arguments
    name.  The definition is from_rgb01_any(utils.image.resize(x, size, filter), ...): the resized values are not clamped before the
    conversion clamps them.  Device tensors: one launch of lvae_resample_f32_to_yuv per 16 images gives those bits with no fp32 image in
    between; outs: frames of that kind and size on the images' device to write instead of new ones -- their planes may be views of larger
    tensors (unit column stride), and nothing outside them is written.  CPU tensors take that composition of the two CPU paths.  ValueError: images of different sizes, a size that does not fit
    the subsampling (it is named), a layout these parameters do not have, an unknown filter, a ratio outside [1/8, 8]."""
    from .. import _native
    from . import resample
    from .image import resize
    from .views import strided_batch
    who = 'from_rgb01_scaled'
    _check2(range=range)
    resample._filter(filter)
    fmt = FrameFormat(layout, depth, subsampling, siting, matrix)
    vs = _rgb_items(xs, None, who)
    h_in, w_in = int(vs[0].shape[1]), int(vs[0].shape[2])
    if any(tuple(v.shape) != (3, h_in, w_in) for v in vs):
        raise ValueError(f'{who}: the images of one call share one size')
    h, w = int(size[0]), int(size[1])
    if not _extent_ok(h, w, subsampling):
        raise ValueError(f'{who}: size {(h, w)} does not fit subsampling {subsampling}')
    resample.check_ratio(h_in, h)
    resample.check_ratio(w_in, w)
    device = vs[0].device
    if device.type == 'cpu':
        x = resize(torch.stack([v.to(torch.float32) for v in vs]), (h, w), filter)
        return from_rgb01_any(x, None, depth, subsampling, siting, matrix, range, layout)
    B = len(vs)
    if outs is None:
        outs = [fmt.new(h, w, device) for _ in vs]
    elif len(outs) != B or any(FrameFormat.of(f) != fmt or f.size != (h, w) or f.device != device for f in outs):
        raise ValueError(f'{who}: outs holds one frame of {h} x {w} per image, on {device}, with the layout, depth and subsampling asked for')
    elif any(p.stride(-1) != 1 or (p.dim() == 3 and p.stride(1) != 2) for f in outs for p in f.planes()):
        raise ValueError(f'{who}: the planes of outs have unit column stride')
    codes, names, lay = _kind_codes(fmt, siting, matrix, range)
    tabs, _ = _scaled_tables((h_in, w_in), (h, w), filter, device)
    with torch.cuda.device(device):
        keep, px, (s_img, s_plane, s_row) = strided_batch(vs, h_in, w_in, device)
        if B > 1 and s_img < 2 * s_plane + (h_in - 1) * s_row + w_in:      # views that overlap as a batch are packed instead
            keep, px, (s_img, s_plane, s_row) = strided_batch([v.clone() for v in vs], h_in, w_in, device)
        ptrs, rows, hw, _ = _plane_args(outs, names)
        _native.check(_native.lib().lvae_resample_f32_to_yuv(px, s_img if B > 1 else 3 * s_plane, s_plane, s_row, hw, B, *codes, lay, h_in, w_in,
                                                             h, w, *tabs, *ptrs, *rows, _stream(device)), 'resample_f32_to_yuv')
    del keep
    return outs


# ----------------------------------------------------------------------------------------------- tiled images straight into YUV planes
def check_chroma_box(box, subsampling, who):
    """ValueError unless box = (y0, x0, hh, ww) starts and ends on the chroma grid of `subsampling`: its frame then has whole chroma
    samples, and they are the full frame's."""
    y0, x0, hh, ww = box
    sx, sy = SHIFTS[subsampling]
    if (sy and (y0 % 2 or hh % 2)) or (sx and (x0 % 2 or ww % 2)):
        raise ValueError(f'{who}: box {tuple(box)} is off the chroma grid of {subsampling}: '
                         f"{'rows and columns' if sy else 'columns'} must start and end on even numbers")


def new_frame(h, w, device, depth=8, subsampling='420', layout='planar'):
    """FrameFormat(layout, depth, subsampling).new(h, w, device)."""
    return FrameFormat(layout, depth, subsampling).new(h, w, device)


def stitch_tiles_yuv(tiles, h, w, th, tw, overlap, box=None, depth=8, subsampling='420', siting='center', matrix='bt709', range='limited',
                     layout='planar', out=None):
    """utils.image.stitch_tiles followed by from_rgb01_any, as ONE kernel (lvae_tile_stitch_yuv: one small copy and one launch on the
    current stream) and with the same bits: a window of a tiled (h, w) image as a frame of the window's size on the tiles' device, with no
    fp32 image in between.  tiles, h, w, th, tw, overlap, box: as in stitch_tiles.  depth .. range: as in from_rgb01_any.  layout: 'planar'
    (-> YuvFrame), 'semiplanar' (-> YuvSpFrame: 10 | 12 bits at '420' | '422'), 'i420' / 'nv12' (-> Yuv420Frame: 8 bits, '420', 'center',
    'bt601' | 'bt709').  A window is the crop of the whole frame: with siting='left' and x0 > 0 its first chroma column reads column x0 - 1
    of the IMAGE, so the tiles holding that column must be there too.  out: a frame of that kind and size on the tiles' device to write
    instead of a new one; its planes may be views of larger tensors (unit column stride), and nothing outside them is written.
    ValueError: what stitch_tiles raises; a box off the chroma grid (odd y0 / hh at '420', odd x0 / ww at '420' / '422'); a layout the
    depth, subsampling, siting or matrix does not have; a tile that is None but meets the box (widened by column x0 - 1 as above)."""
    from .. import _native
    from .image import _stitch_args
    from .tiling import tiles_in_box
    who = 'stitch_tiles_yuv'
    _check2(range=range)
    fmt = FrameFormat(layout, depth, subsampling, siting, matrix)
    box = (0, 0, int(h), int(w)) if box is None else tuple(int(v) for v in box)
    check_chroma_box(box, subsampling, who)
    ys, xs, (y0, x0, hh, ww), t0, addr, oy, ox = _stitch_args(tiles, h, w, th, tw, overlap, box, who)
    if y0 < 0 or x0 < 0 or hh <= 0 or ww <= 0 or y0 + hh > h or x0 + ww > w:
        raise ValueError(f'{who}: box {box} is not inside the {h} x {w} image')
    xl = x0 - 1 if siting == 'left' and SHIFTS[subsampling][0] and x0 > 0 else x0
    missing = [k for k in tiles_in_box(ys, xs, th, tw, (y0, xl, hh, x0 + ww - xl)) if tiles[k] is None]
    if missing:
        raise ValueError(f'{who}: tiles {missing} were not decoded but meet the box {box}' + (' widened by the column before it' if xl < x0 else ''))
    device = t0.device
    if out is None:
        out = fmt.new(hh, ww, device)
    elif FrameFormat.of(out) != fmt or out.size != (hh, ww) or out.device != device:
        raise ValueError(f'{who}: out is a frame of {hh} x {ww} on {device} with the layout, depth and subsampling asked for')
    sp = fmt.interleaved                                     # NV12 as well: for the kernel both are a plane of (U, V) pairs
    y, u, v = out.planes() + ((None,) if sp else ())
    for p in (y, u, v):
        if p is not None and (p.stride(-1) != 1 or (p.dim() == 3 and p.stride(1) != 2)):
            raise ValueError(f'{who}: the planes of out have unit column stride')
    lib = _native.lib()
    with torch.cuda.device(device):
        nbytes = lib.lvae_tile_stitch_workspace_bytes(len(ys), len(xs))
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
        _native.check(lib.lvae_tile_stitch_yuv(addr, t0.stride(0), t0.stride(1), oy, ox, len(ys), len(xs), th, tw, overlap, h, w, y0, x0, hh, ww,
                                               depth, SUBSAMPLINGS.index(subsampling), SITINGS.index(siting), MATRICES2.index(matrix),
                                               RANGES.index(range), LAYOUTS.index('semiplanar' if sp else 'planar'), y.data_ptr(), u.data_ptr(),
                                               None if sp else v.data_ptr(), y.stride(0), u.stride(0), 0 if sp else v.stride(0), ws.data_ptr(),
                                               nbytes, _stream(device)), 'tile_stitch_yuv')
    return out

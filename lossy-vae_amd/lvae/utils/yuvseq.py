"""The self-describing container of a coded YUV sequence, `LVYS`, host side.  Pure Python, no GPU (as utils/tiling.py for `LVTL`): the
models' compress_yuv_sequence / decompress_yuv_sequence (lvae/models/base.py) code each frame through compress_yuv / decompress_yuv and
keep the frames' blobs -- the models' own containers, unchanged -- inside this one, next to everything a decoder otherwise has to be
told: frame size, depth, subsampling, siting, matrix, range, the encoder's chroma filter, the plane layout of the source, the model's name
and the GEMM arithmetic that wrote the streams.  A table of byte lengths in front of the blobs gives random access to a frame.

Layout, little-endian:
    4s magic 'LVYS' | B version | B reserved (0) | I width | I height | B depth | B subsampling | B siting | B matrix | B range | B chroma |
    B layout | B len(model) | B len(gemm) | I frames | model name | GEMM precision name | frames x I byte length | the frames' blobs
The one-byte codes are indexes into the tuples below (the LVAE_YUV_* codes of include/lvae_hip.h where there is one).
"""
import struct

MAGIC = b'LVYS'
VERSION = 1
_HEAD = '<4sBBIIBBBBBBBBBI'
HEAD_BYTES = struct.calcsize(_HEAD)

DEPTHS = (8, 10, 12)
SUBSAMPLINGS = ('420', '422', '444')
SITINGS = ('center', 'left')
MATRICES = ('bt601', 'bt709', 'bt2020')
RANGES = ('limited', 'full')
CHROMA = ('nearest', 'bilinear')
LAYOUTS = ('planar', 'semiplanar', 'i420', 'nv12')          # 'i420' / 'nv12': the 8-bit 4:2:0 frames of utils.yuv.Yuv420Frame
FIELDS = ('width', 'height', 'depth', 'subsampling', 'siting', 'matrix', 'range', 'chroma', 'layout', 'model', 'gemm')


def is_yuv_sequence(blob):
    return bytes(blob[:4]) == MAGIC


def check_layout(layout, depth, subsampling, siting='center', matrix='bt709'):
    """ValueError unless frames of `layout` exist at these parameters.  THE statement of that rule: utils.yuv.FrameFormat, the models'
    YUV entry points and this container all ask here."""
    for v, known, what in ((layout, LAYOUTS, 'layout'), (depth, DEPTHS, 'depth'), (subsampling, SUBSAMPLINGS, 'subsampling'),
                           (siting, SITINGS, 'siting'), (matrix, MATRICES, 'matrix')):
        if v not in known:
            raise ValueError(f'{what} is one of {known}, got {v!r}')
    if layout == 'semiplanar' and (depth not in (10, 12) or subsampling not in ('420', '422')):
        raise ValueError(f'semi-planar frames are 10 / 12 bits at 4:2:0 / 4:2:2, got {depth} bits at {subsampling}')
    if layout in ('i420', 'nv12') and ((depth, subsampling, siting) != (8, '420', 'center') or matrix == 'bt2020'):
        raise ValueError(f"{layout} frames are 8 bits at 4:2:0 with siting 'center' and bt601 / bt709, got {depth} bits at {subsampling}, "
                         f'siting {siting!r}, {matrix}')


def _extent_ok(h, w, subsampling):
    return h > 0 and w > 0 and (subsampling == '444' or w % 2 == 0) and (subsampling != '420' or h % 2 == 0)


def pack_sequence(meta, blobs):
    """meta: a dict with the keys FIELDS (names, not codes) -> the container around `blobs`, one per frame in display order.  ValueError:
    a value outside its tuple, a size that does not fit the subsampling, a layout that does not exist at these parameters, a name
    beyond 255 bytes, a blob beyond 4 GiB."""
    missing = [k for k in FIELDS if k not in meta]
    if missing:
        raise ValueError(f'pack_sequence: missing {missing}')
    codes = []
    for key, known in (('depth', DEPTHS), ('subsampling', SUBSAMPLINGS), ('siting', SITINGS), ('matrix', MATRICES), ('range', RANGES),
                       ('chroma', CHROMA), ('layout', LAYOUTS)):
        if meta[key] not in known:
            raise ValueError(f'pack_sequence: {key} is one of {known}, got {meta[key]!r}')
        codes.append(known.index(meta[key]))
    w, h = int(meta['width']), int(meta['height'])
    if not _extent_ok(h, w, meta['subsampling']) or max(w, h) > 0xffffffff:
        raise ValueError(f'pack_sequence: {w} x {h} does not fit subsampling {meta["subsampling"]}')
    check_layout(meta['layout'], meta['depth'], meta['subsampling'], meta['siting'], meta['matrix'])
    model, gemm = str(meta['model']).encode('ascii'), str(meta['gemm']).encode('ascii')
    if not model or not gemm or len(model) > 255 or len(gemm) > 255:
        raise ValueError('pack_sequence: the model and GEMM precision names hold 1 .. 255 ASCII bytes')
    blobs = [bytes(b) for b in blobs]
    if any(len(b) > 0xffffffff for b in blobs):
        raise ValueError('pack_sequence: a frame beyond 4 GiB')
    head = struct.pack(_HEAD, MAGIC, VERSION, 0, w, h, *codes, len(model), len(gemm), len(blobs))
    return head + model + gemm + struct.pack(f'<{len(blobs)}I', *[len(b) for b in blobs]) + b''.join(blobs)


def yuv_sequence_info(blob):
    """The header of a container -> dict(FIELDS..., version, frames, lengths, offsets): names for the codes, the frames' byte lengths and
    where each blob starts.  No frame is touched.  ValueError -- nothing is ever decoded from such a blob: bad magic, unknown version, a
    code outside its tuple, a size or layout that does not fit, names or a length table that exceed the blob, lengths that do not add
    up to the blob (a truncated or padded file)."""
    blob = memoryview(blob) if not isinstance(blob, memoryview) else blob
    if len(blob) < 4 or bytes(blob[:4]) != MAGIC:
        raise ValueError('not a YUV sequence container (bad magic)')
    if len(blob) < HEAD_BYTES:
        raise ValueError('YUV sequence container: truncated header')
    _, version, _reserved, w, h, *codes, n_model, n_gemm, count = struct.unpack_from(_HEAD, blob, 0)
    if version != VERSION:
        raise ValueError(f'YUV sequence container version {version}, expected {VERSION}')
    info = dict(version=version, width=w, height=h)
    for key, known, code in zip(('depth', 'subsampling', 'siting', 'matrix', 'range', 'chroma', 'layout'),
                                (DEPTHS, SUBSAMPLINGS, SITINGS, MATRICES, RANGES, CHROMA, LAYOUTS), codes):
        if code >= len(known):
            raise ValueError(f'YUV sequence container: {key} code {code} is not one of {len(known)}')
        info[key] = known[code]
    if not _extent_ok(h, w, info['subsampling']):
        raise ValueError(f'YUV sequence container: {w} x {h} does not fit subsampling {info["subsampling"]}')
    try:
        check_layout(info['layout'], info['depth'], info['subsampling'], info['siting'], info['matrix'])
    except ValueError as e:
        raise ValueError(f'YUV sequence container: bad header ({e})') from None
    o = HEAD_BYTES
    if n_model == 0 or n_gemm == 0 or len(blob) < o + n_model + n_gemm:
        raise ValueError('YUV sequence container: truncated names')
    try:
        info['model'] = bytes(blob[o:o + n_model]).decode('ascii')
        info['gemm'] = bytes(blob[o + n_model:o + n_model + n_gemm]).decode('ascii')
    except UnicodeDecodeError:
        raise ValueError('YUV sequence container: names are not ASCII') from None
    o += n_model + n_gemm
    if len(blob) - o < 4 * count:
        raise ValueError('YUV sequence container: the length table exceeds the blob')
    lengths = list(struct.unpack_from(f'<{count}I', blob, o))
    o += 4 * count
    if o + sum(lengths) != len(blob):
        raise ValueError(f'YUV sequence container: frame lengths add up to {o + sum(lengths)} bytes, the blob has {len(blob)}')
    offsets = []
    for ln in lengths:
        offsets.append(o)
        o += ln
    info.update(frames=count, lengths=lengths, offsets=offsets)
    return info


def frame_indexes(info, frames=None):
    """`frames` of decompress_yuv_sequence -> a list of frame numbers: None = all, a range, or any iterable of indexes (negative ones count
    from the end).  IndexError outside the sequence."""
    n = info['frames']
    if frames is None:
        return list(range(n))
    out = []
    for k in frames:
        k = int(k)
        if not -n <= k < n:
            raise IndexError(f'frame {k} of a sequence of {n}')
        out.append(k % n)
    return out


def frame_blob(blob, info, k):
    """Frame k's bytes: one slice, through the length table."""
    o = info['offsets'][k]
    return bytes(blob[o:o + info['lengths'][k]])


def unpack_sequence(blob):
    """Inverse of pack_sequence -> (the info dict, every frame's bytes)."""
    info = yuv_sequence_info(blob)
    return info, [frame_blob(blob, info, k) for k in range(info['frames'])]


def code_sequence(compress, frames, max_batch=8, lmb=None):
    """The batching of compress_yuv_sequence, apart from any model: compress(chunk, lmb=...) -> one blob per frame, for chunks of
    `max_batch` frames in order.  frames: a list, or a callable (start, count) -> list that returns [] behind the last frame (a raw file
    read `max_batch` frames at a time).  lmb: None, one value, or one value per frame."""
    step = max(1, int(max_batch))
    per_frame = lmb is not None and not isinstance(lmb, (int, float))
    if per_frame:
        lmb = [float(v) for v in lmb]
    blobs, start = [], 0
    while True:
        chunk = frames(start, step) if callable(frames) else frames[start:start + step]
        if not chunk:
            break
        if per_frame and start + len(chunk) > len(lmb):
            raise ValueError(f'{len(lmb)} lambdas for a sequence of more than {start + len(chunk) - 1} frames')
        kw = {} if lmb is None else {'lmb': lmb[start:start + len(chunk)] if per_frame else lmb}
        got = compress(chunk, **kw)
        if len(got) != len(chunk):
            raise ValueError(f'{len(got)} blobs for {len(chunk)} frames')
        blobs += got
        start += len(chunk)
    if per_frame and len(lmb) != start:
        raise ValueError(f'{len(lmb)} lambdas for {start} frames')
    return blobs

"""Lists of image tensors as the native entries address them: (C, h, w) views, and one base pointer + (image, plane, row) strides for
views cut from one tensor (shared by lvae.metrics and lvae.utils.image)."""
import torch


def items(t, name):
    """A (B, C, H, W) tensor or a list of (1, C, h, w) / (C, h, w) tensors -> list of (C, h, w) views."""
    if torch.is_tensor(t):
        if t.dim() != 4:
            raise ValueError(f'{name}: expected a (B, C, H, W) tensor or a list of images, got shape {tuple(t.shape)}')
        return [t[i] for i in range(t.shape[0])]
    out = []
    for v in t:
        if v.dim() == 4 and v.shape[0] == 1:
            v = v[0]
        if v.dim() != 3:
            raise ValueError(f'{name}: list items are (1, C, h, w) or (C, h, w) tensors, got shape {tuple(v.shape)}')
        out.append(v)
    return out


def strided_batch(items, hmax, wmax, device):
    """Address a list of (C, h_i, w_i) images as ONE base pointer + (image, plane, row) strides in elements.  Views cut from one tensor
    with a common spacing (what decompress_files returns: out[i:i+1, :, :h, :w]) are used where they lie; anything else (CPU tensors,
    separately allocated images, another dtype) is packed into one zero-padded (B, C, hmax, wmax) fp32 tensor on the device.
    Returns (keep-alive tensor, data_ptr, strides)."""
    v0 = items[0]
    ok = all(v.device == device and v.dtype == torch.float32 and v.stride(2) == 1 and v.stride()[:2] == v0.stride()[:2]
             and v.untyped_storage().data_ptr() == v0.untyped_storage().data_ptr() for v in items)
    if ok:
        plane, row = v0.stride(0), v0.stride(1)
        step = (items[1].data_ptr() - v0.data_ptr()) // 4 if len(items) > 1 else 0
        ok = all(v.data_ptr() - v0.data_ptr() == 4 * step * i for i, v in enumerate(items)) and (len(items) == 1 or step > 0)
        # the extents have to fit the strides (an expanded or overlapping view does not): the native entry checks the same
        ok = ok and all(v.shape[2] <= row and (v.shape[1] - 1) * row + v.shape[2] <= plane for v in items)
        if ok:
            return items, v0.data_ptr(), (step, plane, row)
    C = v0.shape[0]
    buf = torch.zeros(len(items), C, hmax, wmax, dtype=torch.float32, device=device)
    for i, v in enumerate(items):
        buf[i, :, :v.shape[1], :v.shape[2]].copy_(v, non_blocking=True)
    return buf, buf.data_ptr(), (C * hmax * wmax, hmax * wmax, wmax)

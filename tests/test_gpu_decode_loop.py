"""gpu: the per-block Python decode loop the two codecs share (CodecBase._decode_group_loop) against the default path, without
(qarv_base) and with (qres34m_lossless) the per-block override for the output net's pixel stream."""
import pytest
import torch

import lvae
import seeded_init
from conftest import load_seeded_into
from oracle import qres_oracle


def _batch(n, h, w):
    return torch.cat([torch.from_numpy(seeded_init.synthetic_image_u8(h, w, 70 + i)).permute(2, 0, 1).float().div(255).unsqueeze(0)
                      for i in range(n)], 0).cuda()


@pytest.fixture(scope='module')
def lossless_model():
    sd = seeded_init.seeded_state_dict(qres_oracle.qres_param_shapes(qres_oracle.qres34m_lossless_arch()), seed=0)
    m = load_seeded_into(lvae.get_model('qres34m_lossless'), sd)
    m.compress_mode()
    return m.to('cuda:0').eval()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['qarv_base', 'qres34m_lossless'])
def test_python_decode_loop_equals_default_and_single_image_decodes(name, request):
    """B = 5 at 64x128 (two pipeline groups, of 3 and 2 images): decompress_batch with native_group_loops = False returns the bits
    of the default path, and each row the bits of decompress() of that image's stream."""
    m = request.getfixturevalue('product_model' if name == 'qarv_base' else 'lossless_model')
    ims = _batch(5, 64, 128)
    streams = m.compress_batch(ims)
    assert [n for _, n in m._groups(5, 'dec')] == [3, 2]
    x = m.decompress_batch(streams).clone()
    try:
        m.native_group_loops = False
        x_py = m.decompress_batch(streams).clone()
    finally:
        m.native_group_loops = True
    assert torch.equal(x_py, x)
    for b in range(5):
        assert torch.equal(m.decompress(streams[b])[0], x[b]), b
    if name == 'qres34m_lossless':
        assert torch.equal(torch.round(x * 255), torch.round(ims * 255))

"""Alpha-weighted histograms for RGBA training (Trainer / FolderData `hist_alpha_weight`, opt-in): the colour stored under
transparent pixels stops counting in the target histograms and in the generator-side histogram of the G loss."""
import numpy as np
import pytest
import torch

from conftest import relmax

pytestmark = pytest.mark.gpu


def _rgba_folder(path, n=3, size=40):
    from PIL import Image
    rs = np.random.RandomState(0)
    for i in range(n):
        img = rs.randint(0, 256, (size, size, 4)).astype(np.uint8)
        img[:, size // 2:, 3] = 0
        Image.fromarray(img, 'RGBA').save(path / f'{i}.png')


def test_rgba_steps_with_alpha_weighted_histograms(gpu_device, tmp_path):
    """The size of test_trainer_io_gpu.py::test_transparent_rgba_steps: synthetic data, then an RGBA folder."""
    from histoGAN import Trainer
    tr = Trainer('rgbaw', str(tmp_path / 'r'), str(tmp_path / 'm'), 32, 2, transparent=True, batch_size=2, hist_bin=16,
                 hist_insz=32, hist_resizing='interpolation', hist_alpha_weight=True)
    assert tr.hist_alpha_weight is True
    tr.run_evaluate = tr.run_save = False
    tr.set_synthetic_data_src()
    for _ in range(3):
        tr.train(alpha=2)
    assert np.isfinite(tr.d_loss) and np.isfinite(tr.g_loss) and np.isfinite(tr.h_loss)
    (tmp_path / 'data').mkdir()
    _rgba_folder(tmp_path / 'data')
    tr.set_data_src(str(tmp_path / 'data'))
    assert tr.loader.alpha_weight and tr.loader_evaluate.alpha_weight
    for _ in range(2):
        tr.train(alpha=2)
    assert np.isfinite(tr.d_loss) and np.isfinite(tr.g_loss) and np.isfinite(tr.h_loss)


def test_alpha_weight_needs_transparent(gpu_device, tmp_path):
    from histoGAN import Trainer
    with pytest.raises(ValueError, match='transparent'):
        Trainer('bad', str(tmp_path / 'r'), str(tmp_path / 'm'), 32, 2, transparent=False, batch_size=2, hist_bin=16,
                hist_insz=32, hist_alpha_weight=True)
    tr = Trainer('off', str(tmp_path / 'r'), str(tmp_path / 'm'), 32, 2, transparent=True, batch_size=2, hist_bin=16, hist_insz=32)
    assert tr.hist_alpha_weight is False


def test_folderdata_alpha_weighted_target_is_the_opaque_half(gpu_device, tmp_path):
    """An RGBA image whose transparent half is painted a strong colour: with the flag the target histogram equals the
    oracle's histogram of the opaque half alone (binary mask == the selected pixels), without it the paint counts."""
    from PIL import Image
    from histogan_amd.data import FolderData
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    from oracle import rgbuv_hist as O
    rs = np.random.RandomState(1)
    img = np.zeros((24, 32, 4), np.uint8)
    img[..., :3] = rs.randint(0, 256, (24, 32, 3))
    img[:, 16:, :3] = (255, 64, 128)
    img[:, :16, 3] = 255
    Image.fromarray(img, 'RGBA').save(tmp_path / 'a.png')
    opaque = torch.from_numpy(img[:, :16, :3].astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    for method in ('inverse-quadratic', 'thresholding'):
        blk = RGBuvHistBlock(h=16, insz=64, method=method, device='cuda')
        ref = O.rgbuv_hist(opaque, h=16, insz=64, method=method).numpy()
        on = FolderData(str(tmp_path), blk, 1, 8, gpu_device, transparent=True, test=True, hist_alpha_weight=True)
        off = FolderData(str(tmp_path), blk, 1, 8, gpu_device, transparent=True, test=True)
        h_on, h_off = next(on)['histograms'].cpu().numpy(), next(off)['histograms'].cpu().numpy()
        assert relmax(h_on, ref) <= 1e-5
        assert relmax(h_off, ref) > 1e-2

"""Projection of an image into HistoGAN's latent space, and recolouring of the projected image.

What the reference does in projection_gaussian.py / projection_to_latent.py (project_to_latent :197-570, process_image
:71-106, recolor_image :109-194), restated on this package's generator: the averaged networks SE, HE and GE stay fixed
and Adam moves the generator's INPUTS -- one style row per block below the two histogram blocks, and the noise -- until
GE reproduces the image; the histogram embedding comes from the image's own RGB-uv histogram through HE, so that the
projected image can afterwards be rendered with any other histogram (`recolor`).

With the noise image as the variable (optimize_noise, not latent_noise) a step is ONE call of GE, served by the one-node
training pass (gfused.py) with frozen weights: its backward returns the style and noise-image gradients
(hg_noise_grad, include/hg_nets.h) and launches no weight-gradient convolution.  With latent_noise the variables are
the per-layer noise feature maps, fed through GeneratorBlock.forward_(noise1=, noise2=) -- plain autograd, as before.

Not here: the VGG perceptual term (see `project`; the weight-free perceptual colour term in its place is the CIE colour
difference, `delta_e_weight`, and SSIM / MS-SSIM of the lightness plane, `ssim_weight`), face_preprocessing, command-line front ends and file I/O.  The caller
post-processes `recolor`'s output with post.pyramid_upsampling / post.color_transfer_mkl as the reference's scripts do, or
with post.color_transfer_idt (recoloringTrainer.evaluate's post_recoloring='idt'), the nonlinear transfer, where the
recoloured image's whole colour distribution is wanted on the photo and not only its mean and covariance, or with
post.color_transfer_palette (post_recoloring='palette'), the third transfer: post.paired_palette of the projected image and
its recolouring gives K paired colours, and every pixel of the photo moves by a smooth blend of their shifts.
"""
import torch
import torch.nn.functional as F


def _freeze(*modules):
    for m in modules:
        for p in m.parameters():
            p.requires_grad_(False)


def _render(GAN, styles, h_w, in_noise=None, noise1_list=None, noise2_list=None):
    """process_image (:71-106): block i < L - 2 takes SE(styles[:, i]), the last two take the histogram embedding h_w."""
    GE, SE = GAN.GE, GAN.SE
    n_rows = len(GE.blocks) - 2
    if noise1_list is None or noise2_list is None:
        w = torch.stack([SE(styles[:, i, :]) for i in range(n_rows)], dim=1)
        return GE(w, torch.stack((h_w, h_w), dim=1), in_noise)
    x = GE.initial_block.expand(styles.shape[0], -1, -1, -1)
    rgb = None
    for i, (n1, n2, block) in enumerate(zip(noise1_list, noise2_list, GE.blocks)):
        s = SE(styles[:, i, :]) if i < n_rows else h_w
        x, rgb = block.forward_(x, rgb, block.to_style1(s), block.to_style2(s), block.to_rgb.to_style(s), noise1=n1, noise2=n2)
    return rgb


def project(GAN, image, steps=1000, lr=0.1, pixel_loss='L1', pixel_loss_weight=1.0, optimize_noise=True, latent_noise=False,
            noise_reg_weight=0.0, style_reg_weight=0.0, hist_block=None, seed=None, vgg_loss_weight=0.0, hist=None,
            delta_e_weight=0.0, delta_e_kind='2000', ssim_weight=0.0, ssim_kind='ssim'):
    """Adam on [styles] (+ the noise) against the frozen SE / HE / GE of `GAN` until GE reproduces `image`.

    image: (B, 3, S, S) in [0, 1] on the generator's device.  hist_block: the histogram module that gives the image's own
    histogram (RGBuvHistBlock); or pass the histogram itself as `hist` (B, 3, h, h).  optimize_noise + latent_noise: the
    variables are the per-layer noise maps to_noise_k(in_noise), else the noise image in_noise (optimize_noise) or the
    styles alone.  seed: of the draw of the latent and the noise image (None: the global generator).

    Per step (:466-504):  pixel_loss_weight * (L1 | L2)(image, rgb) + noise_reg_weight * mean(noise)^2 (latent_noise: the
    sum over both maps of a layer, averaged over the layers) + style_reg_weight * mean(styles)^2 / rows
    + delta_e_weight * mean_b(post.delta_e(rgb, image, delta_e_kind)) when delta_e_weight is not 0: the CIE colour difference
    ('2000': CIEDE2000, '76': dE76) as the perceptual colour term, where the reference has its VGG loss.  dE is in Lab units --
    a few units for a fair reproduction, against a pixel term of a few hundredths -- so a useful delta_e_weight is around 1e-2
    of pixel_loss_weight.  With the default 0 nothing of it is launched.
    + ssim_weight * mean_b(1 - post.ssim(rgb, image)) when ssim_weight is not 0: the structure of the lightness plane,
    independent of its colour; ssim_kind='ms-ssim' takes post.ms_ssim instead and needs image_size >= 176.  With the default 0
    nothing of it is launched.

    Returns (data, losses, rgb): the dict the reference pickles -- {'styles', 'in_noise'} or {'styles', 'noise1_list',
    'noise2_list'} --, the loss of every step (floats) and the image rendered from `data`, which
    recolor(GAN, data, <the same histogram>) reproduces."""
    if vgg_loss_weight:
        raise NotImplementedError(
            'project: vgg_loss_weight must be 0 -- the perceptual loss needs VGG16\'s trained weights, which are not part of '
            'the reference tree (torchvision downloads them), and a perceptual loss on random weights verifies nothing')
    if pixel_loss not in ('L1', 'L2'):
        raise ValueError('pixel loss should be either L1 or L2')
    if delta_e_weight:
        from . import post
        delta_e_kind = post.delta_e_kind(delta_e_kind, 'project')          # ValueError before a device is touched
    if ssim_weight:
        from . import post
        if ssim_kind not in ('ssim', 'ms-ssim'):                            # ValueError before a device is touched
            raise ValueError(f"project: ssim_kind must be 'ssim' or 'ms-ssim', not {ssim_kind!r}")
        if ssim_kind == 'ms-ssim' and GAN.GE.image_size < post.MS_SSIM_MIN_SIZE:
            raise ValueError(f'project: ssim_kind=\'ms-ssim\' needs image_size >= {post.MS_SSIM_MIN_SIZE}, got {GAN.GE.image_size}')
        ssim_fn = post.ms_ssim if ssim_kind == 'ms-ssim' else post.ssim
    if hist is None and hist_block is None:
        raise ValueError('project: give the histogram block (hist_block) or the image\'s histogram (hist)')
    GE = GAN.GE
    _freeze(GAN.SE, GAN.HE, GE)
    dev = image.device
    B, S, n_rows = image.shape[0], GE.image_size, GE.num_layers - 2
    image = image.detach()
    gen = None if seed is None else torch.Generator().manual_seed(seed)
    # one latent, repeated over the style rows (:407-410), and one noise image (:411), drawn on the host
    styles = torch.randn(B, GE.latent_dim, generator=gen)[:, None, :].repeat(1, n_rows, 1).to(dev).requires_grad_()
    in_noise = torch.rand(B, S, S, 1, generator=gen).to(dev)
    with torch.no_grad():
        h_w = GAN.HE(hist_block(image) if hist is None else hist)
    noise1_list = noise2_list = None
    if optimize_noise and latent_noise:
        noise1_list, noise2_list = [], []
        with torch.no_grad():
            for i, block in enumerate(GE.blocks):
                nz = in_noise[:, :4 << i, :4 << i, :]
                noise1_list.append(block.to_noise1(nz).permute(0, 3, 2, 1).contiguous().requires_grad_())
                noise2_list.append(block.to_noise2(nz).permute(0, 3, 2, 1).contiguous().requires_grad_())
        variables = [styles] + noise1_list + noise2_list
        in_noise = None
    elif optimize_noise:
        in_noise.requires_grad_()
        variables = [styles, in_noise]
    else:
        variables = [styles]
    opt = torch.optim.Adam(variables, lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        rgb = _render(GAN, styles, h_w, in_noise, noise1_list, noise2_list)
        rec = torch.mean(torch.abs(image - rgb)) if pixel_loss == 'L1' else F.mse_loss(image, rgb)
        loss = pixel_loss_weight * rec
        if delta_e_weight:
            loss = loss + delta_e_weight * post.delta_e(rgb, image, delta_e_kind).mean()
        if ssim_weight:
            loss = loss + ssim_weight * (1.0 - ssim_fn(rgb, image)).mean()
        if optimize_noise and latent_noise:
            reg = sum(n1.mean() ** 2 + n2.mean() ** 2 for n1, n2 in zip(noise1_list, noise2_list))
            loss = loss + noise_reg_weight * reg / len(noise1_list)
        elif optimize_noise:
            loss = loss + noise_reg_weight * in_noise.mean() ** 2
        loss = loss + style_reg_weight * styles.mean() ** 2 / styles.shape[1]
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]        # (one host synchronisation after the loop, not one per step)
    if in_noise is None:
        data = {'styles': styles, 'noise1_list': noise1_list, 'noise2_list': noise2_list}
    else:
        data = {'styles': styles, 'in_noise': in_noise}
    return data, losses, recolor(GAN, data, h_w=h_w)


def recolor(GAN, data, target_hist=None, add_noise=False, random_styles=(), h_w=None):
    """The generate half (recolor_image :109-194): GE on the projected `data` with the histogram `target_hist`
    (B, 3, h, h) in place of the image's own.  add_noise: the stored noise image is averaged with a fresh one (:144-147).
    random_styles: 1-based style rows to replace by one fresh latent each (:125-133).  `data` is not modified."""
    GE = GAN.GE
    styles = data['styles'].detach()
    if random_styles:
        rows = sorted(set(int(i) for i in random_styles))
        if rows[0] < 1 or rows[-1] > GE.num_layers - 2:
            raise ValueError('random_styles: rows are numbered 1 .. num_layers - 2')
        styles = styles.clone()
        for i in rows:
            styles[:, i - 1, :] = torch.randn(styles.shape[0], styles.shape[2]).to(styles.device)
    in_noise = n1 = n2 = None
    if 'in_noise' in data:
        in_noise = data['in_noise'].detach()
        if add_noise:
            in_noise = (in_noise + torch.rand(in_noise.shape).to(in_noise.device)) / 2
    else:
        n1, n2 = [t.detach() for t in data['noise1_list']], [t.detach() for t in data['noise2_list']]
    with torch.no_grad():
        if h_w is None:
            h_w = GAN.HE(target_hist)
        return _render(GAN, styles, h_w, in_noise, n1, n2)

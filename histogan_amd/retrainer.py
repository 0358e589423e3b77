"""ReHistoGAN container + trainer on the MI355X path.

API mirror of ReHistoGAN/rehistoGAN.py (reference): `recoloringGAN` (:637-718) and `recoloringTrainer` (:721-1226)
keep their constructor arguments, attribute names (`GAN.{ED,H,G,D,G_opt,D_opt}`, `steps`, ...), method names and
the checkpoint format.  `recoloringTrainer.train(alpha, beta, gamma)` performs the reference's D step + G step
(:895-1073: hinge loss, gradient penalty every 4th step, gamma * adversarial + alpha * Hellinger histogram loss +
beta * L1/Sobel/Laplacian reconstruction loss [+ variance loss], DiffGrad, NaN recovery), restructured as the
HistoGAN trainer is (histogan_amd/trainer.py): flat parameter/gradient buffers with fused DiffGrad, the D phase's
encoder-decoder + head under no_grad (the reference builds and discards that graph), one `[fake; real]`
discriminator pass, no D weight gradients in the G phase, one read-back per step, RCCL all-reduce of the flat
gradient buffers under data parallelism.

Provenance: the step (`train`), `_recolor`, the loss plumbing and the data sources are original.  The API-compatibility
shell -- the `recoloringTrainer.__init__` attribute block, `config` / `write_config` / `load_config`, `print_log`,
`model_name`, `init_folders`, `clear` (all of these but `print_log` are `Trainer`'s own functions), `save`, `load` and
`evaluate`'s parameter list -- follows the reference method for method (ReHistoGAN/rehistoGAN.py:721-893, 1076-1226),
because its CLI, checkpoints and scripts address these names; none of it is on the timed path.  The discriminator phase
and the second-stream forward of the step are `trainer.discriminator_phase` and `trainer.SideStreamForward`.
"""
from math import floor, log2, pi
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ddp, post, reops
from .conv import enable_pack_cache, weights_changed
from .hist import hellinger_loss
from .nets import Discriminator, HistVectorizer
from .optim import DiffGrad, FlatParams
from .renets import RecoloringEncoderDecoder, RecoloringGAN
from .trainer import (NanException, SideStreamForward, SyntheticData, Trainer, _freeze_gc_once, _Rng, cast_list,
                      discriminator_phase, gradient_penalty, set_requires_grad)

SOBEL_X = ((1, 0, -1), (2, 0, -2), (1, 0, -1))
SOBEL_Y = ((1, 2, 1), (0, 0, 0), (-1, -2, -1))
LAPLACIAN = ((0, 1, 0), (1, -4, 1), (0, 1, 0))


def get_gaussian_kernel(kernel_size=15, sigma=3, channels=3):
    """The reference's depthwise Gaussian (:207-225) as its (channels,1,k,k) weight tensor (all slices equal)."""
    x_coord = torch.arange(kernel_size)
    x_grid = x_coord.repeat(kernel_size).view(kernel_size, kernel_size)
    xy_grid = torch.stack([x_grid, x_grid.t()], dim=-1).float()
    mean = (kernel_size - 1) / 2.
    variance = sigma ** 2.
    k = (1. / (2. * pi * variance)) * torch.exp(-torch.sum((xy_grid - mean) ** 2., dim=-1) / (2 * variance))
    k = k / torch.sum(k)
    return k.view(1, 1, kernel_size, kernel_size).repeat(channels, 1, 1, 1)


def gaussian_op(x, kernel=None):
    if kernel is None:
        kernel = get_gaussian_kernel(kernel_size=15, sigma=15, channels=3)
    return reops.gaussian_valid(x, kernel)


def laplacian_op(x, kernel=None):
    return reops.stencil3(x, LAPLACIAN if kernel is None else kernel)


def sobel_op(x, dir=0, kernel=None):
    return reops.stencil3(x, (SOBEL_X if dir == 0 else SOBEL_Y) if kernel is None else kernel)


class reconstruction_loss(object):
    """'L1' | '1st gradient' (Sobel magnitude) | '2nd gradient' (Laplacian); reference :279-326.  'SSIM' (no counterpart in
    the reference): mean_b(1 - post.ssim) of the lightness planes, structure preserved whatever the colours do."""

    def __init__(self, loss):
        self.loss = loss

    def compute_loss(self, input, target):
        if self.loss == 'L1':
            return torch.mean(torch.abs(input - target))
        if self.loss == '1st gradient':
            ig = torch.sqrt(sobel_op(input, 0) ** 2 + sobel_op(input, 1) ** 2)
            tg = torch.sqrt(sobel_op(target, 0) ** 2 + sobel_op(target, 1) ** 2)
            return torch.mean(torch.abs(ig - tg))
        if self.loss == '2nd gradient':
            # the stencil is linear: one pass over the difference image
            return torch.mean(torch.abs(laplacian_op(input - target)))
        if self.loss == 'SSIM':
            # the trainer passes the generated image second, and post.ssim differentiates its first argument
            return torch.mean(1.0 - post.ssim(target[:, :3], input[:, :3]))
        return None


class recoloringGAN(nn.Module):
    def __init__(self, image_size, latent_dim=512, style_depth=8, network_capacity=16, transparent=False, fp16=False,
                 steps=1, lr=1e-4, fq_layers=[], fq_dict_size=256, attn_layers=[], hist=64, skip_conn_to_GAN=False,
                 fixed_gan_weights=False, initialize_gan=False, internal_hist=False, device=None):
        super().__init__()
        if fp16:
            raise NotImplementedError('fp16/apex is not offered: the MI355X path is fp32 (as the reference default)')
        self.lr = lr
        self.steps = steps
        self.fixed_gan_weights = fixed_gan_weights
        self.internal_hist = internal_hist
        self.skip_conn_to_GAN = skip_conn_to_GAN
        self.ED = RecoloringEncoderDecoder(image_size, network_capacity=network_capacity, hist=hist,
                                           latent_dim=latent_dim, style_depth=style_depth,
                                           skip_conn_to_GAN=skip_conn_to_GAN, internal_hist=internal_hist)
        self.H = HistVectorizer(hist, latent_dim, int(style_depth))
        self.G = RecoloringGAN(image_size, latent_dim, network_capacity, transparent=transparent)
        self.D = Discriminator(image_size, network_capacity, fq_layers=fq_layers, fq_dict_size=fq_dict_size,
                               attn_layers=attn_layers, transparent=transparent)
        self._init_weights(initializeGAN=initialize_gan)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.to(device)
        if fixed_gan_weights:
            # the reference leaves G and H out of the optimizer (:672-677); not computing their (unused) gradients
            # is the same update
            set_requires_grad(self.G, False)
            set_requires_grad(self.H, False)
            learnable = list(self.ED.parameters())
        else:
            learnable = list(self.ED.parameters()) + list(self.G.parameters()) + list(self.H.parameters())
        self._flat_g = FlatParams(learnable)
        self._flat_d = FlatParams(self.D.parameters())
        self.G_opt = DiffGrad(self._flat_g, lr=self.lr, betas=(0.5, 0.9))
        self.D_opt = DiffGrad(self._flat_d, lr=self.lr, betas=(0.5, 0.9))
        for f in (self._flat_g, self._flat_d):
            ddp.broadcast_flat(f)
        if fixed_gan_weights and ddp.is_dist():
            for p in list(self.G.parameters()) + list(self.H.parameters()):
                torch.distributed.broadcast(p.data, 0)
        self._reduce_g = ddp.GradAllReduce(self._flat_g)
        self._reduce_d = ddp.GradAllReduce(self._flat_d)
        enable_pack_cache(list(self.ED.parameters()) + list(self.G.parameters()) + list(self.D.parameters()))

    def _init_weights(self, initializeGAN=False):
        if initializeGAN:
            for block in self.G.blocks:
                nn.init.zeros_(block.to_noise1.weight)
                nn.init.zeros_(block.to_noise2.weight)
                nn.init.zeros_(block.to_noise1.bias)
                nn.init.zeros_(block.to_noise2.bias)
            for m in self.H.modules():
                if isinstance(m, (nn.Conv2d, nn.Linear)):
                    nn.init.kaiming_normal_(m.weight, a=0, mode='fan_in', nonlinearity='leaky_relu')
        for net in (self.ED, self.D):
            for m in net.modules():
                if isinstance(m, (nn.Conv2d, nn.Linear)):
                    nn.init.kaiming_normal_(m.weight, a=0, mode='fan_in', nonlinearity='leaky_relu')

    def forward(self, x):
        return x


class recoloringTrainer():
    def __init__(self, name, results_dir, models_dir, image_size, network_capacity, transparent=False, batch_size=4,
                 mixed_prob=0.9, gradient_accumulate_every=1, lr=2e-4, num_workers=None, save_every=1000,
                 trunc_psi=0.6, fp16=False, fq_layers=[], fq_dict_size=256, attn_layers=[],
                 hist_method='inverse-quadratic', hist_resizing='sampling', hist_sigma=0.02, hist_bin=64,
                 hist_insz=150, fixed_gan_weights=False, skip_conn_to_GAN=False, rec_loss='laplacian',
                 initialize_gan=False, variance_loss=True, internal_hist=False, change_hyperparameters=False,
                 change_hyperparameters_after=100000, rng='device', *args, **kwargs):
        from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
        self.GAN_params = [args, kwargs]
        self.GAN = None
        self.hist_method = hist_method
        self.hist_resizing = hist_resizing
        self.hist_sigma = hist_sigma
        self.hist_bin = hist_bin
        self.change_hyperparameters_after = change_hyperparameters_after
        self.hist_insz = hist_insz
        self.rec_loss = rec_loss
        self.internal_hist = internal_hist
        self.change_hyperparameters = change_hyperparameters
        self.variance_loss = variance_loss
        self.fixed_gan_weights = fixed_gan_weights
        self.skip_conn_to_GAN = skip_conn_to_GAN
        self.initialize_gan = initialize_gan
        self.device = torch.device('cuda', torch.cuda.current_device())
        mk = lambda: RGBuvHistBlock(insz=self.hist_insz, h=self.hist_bin, method=self.hist_method,
                                    resizing=self.hist_resizing, sigma=self.hist_sigma)
        self.histBlock = mk()
        if variance_loss is True:
            self.histBlock_input = mk()
            self.gaussKernel = get_gaussian_kernel(kernel_size=15, sigma=5, channels=3).to(self.device)
        if self.rec_loss is None:
            self.rec_loss_func = reconstruction_loss('L1')
        elif self.rec_loss == 'sobel':
            self.rec_loss_func = reconstruction_loss('1st gradient')
        elif self.rec_loss == 'laplacian':
            self.rec_loss_func = reconstruction_loss('2nd gradient')
        elif self.rec_loss == 'ssim':
            self.rec_loss_func = reconstruction_loss('SSIM')
        else:
            raise Exception('Unknown reconstruction losst!')
        self.name = name
        self.results_dir = Path(results_dir)
        self.models_dir = Path(models_dir)
        self.config_path = self.models_dir / name / '.config.json'
        assert log2(image_size).is_integer(), 'image size must be a power of 2 (64, 128, 256, 512, 1024)'
        self.image_size = image_size
        self.network_capacity = network_capacity
        self.transparent = transparent
        self.fq_layers = cast_list(fq_layers)
        self.fq_dict_size = fq_dict_size
        self.attn_layers = cast_list(attn_layers)
        self.lr = lr
        self.batch_size = batch_size
        self.num_workers = num_workers
        self.mixed_prob = mixed_prob
        self.save_every = save_every
        self.steps = 0
        self.av = None
        self.trunc_psi = trunc_psi
        self.gradient_accumulate_every = gradient_accumulate_every
        assert not fp16, 'fp16 is not offered on the MI355X path (fp32 only)'
        self.fp16 = fp16
        self.d_loss = 0
        self.g_loss = 0
        self.last_gp_loss = 0
        self.last_cr_loss = 0
        self.q_loss = 0
        self.r_loss = 0
        self.h_loss = 0
        if self.variance_loss is True:
            self.var_loss = 0
        self.rng = _Rng(self.device, rng)
        self._side = SideStreamForward(self.device)   # the G phase's forward beside the D phase (single-GPU runs)
        self._gc_frozen = False                       # _freeze_gc_once ran
        self.is_main = ddp.rank() == 0
        self.run_evaluate = True
        self.run_save = True
        self.init_folders()
        self.loader = None
        self.loader_evaluate = None

    def init_GAN(self):
        args, kwargs = self.GAN_params
        self.GAN = recoloringGAN(lr=self.lr, image_size=self.image_size, network_capacity=self.network_capacity,
                                 transparent=self.transparent, fq_layers=self.fq_layers,
                                 fq_dict_size=self.fq_dict_size, attn_layers=self.attn_layers, fp16=self.fp16,
                                 hist=self.hist_bin, fixed_gan_weights=self.fixed_gan_weights,
                                 skip_conn_to_GAN=self.skip_conn_to_GAN, initialize_gan=self.initialize_gan,
                                 internal_hist=self.internal_hist, *args, **kwargs)

    # the reference's two trainers spell these six alike, and so do the two here: one copy (they only touch attributes both
    # constructors set, and load_config calls this class's init_GAN)
    write_config, load_config, config = Trainer.write_config, Trainer.load_config, Trainer.config
    model_name, init_folders, clear = Trainer.model_name, Trainer.init_folders, Trainer.clear

    def set_synthetic_data_src(self, pool=4, seed=None):
        seed = ddp.rank() if seed is None else seed
        self.loader = SyntheticData(self.histBlock, self.batch_size, self.image_size, self.device, pool, seed)
        self.loader_evaluate = SyntheticData(self.histBlock, 4, self.image_size, self.device, 1, seed + 977)

    def set_data_src(self, folder, sampling=True, resident=False):
        """resident=True: as Trainer.set_data_src -- data.ResidentFolderData feeds the loader, RGB only."""
        from .data import FolderData, ResidentFolderData
        self.loader = (ResidentFolderData if resident else FolderData)(
            folder, self.histBlock, self.batch_size, self.image_size, self.device, transparent=self.transparent,
            seed=ddp.rank(), hist_sampling=sampling,
            hflip=True)                          # transforms.RandomHorizontalFlip(), ReHistoGAN/rehistoGAN.py:362
        self.loader_evaluate = FolderData(folder, self.histBlock, 4, self.image_size, self.device,
                                          transparent=self.transparent, seed=977 + ddp.rank(),
                                          hist_sampling=sampling)

    # ------------------------------------------------------------------------------------------
    def _recolor(self, image_batch, hist_batch, noise):
        """H -> encoder-decoder -> recolouring head, the four wirings of the reference (:934-952)."""
        GAN = self.GAN
        h_w_space = GAN.H(hist_batch)
        ed_hist = h_w_space if self.internal_hist else hist_batch
        if self.skip_conn_to_GAN:
            image_latent, rgb, latent_a, latent_b = GAN.ED(image_batch, ed_hist)
            return GAN.G(image_latent, rgb, h_w_space, noise, latent_a, latent_b)
        image_latent, rgb = GAN.ED(image_batch, ed_hist)
        return GAN.G(image_latent, rgb, h_w_space, noise)

    def train(self, alpha=32, beta=1.5, gamma=4):
        assert self.loader is not None, ('You must first initialize the data source with '
                                         '`.set_data_src(<folder of images>)` or `.set_synthetic_data_src()`')
        if self.steps >= self.change_hyperparameters_after and self.change_hyperparameters:
            # (the reference assigns self.alpha/gamma/beta here and keeps using the arguments, :900-904)
            self.alpha, self.gamma, self.beta = 8, 2, 1
        torch.autograd.set_detect_anomaly(False)
        if self.GAN is None:
            self.init_GAN()
        GAN = self.GAN
        GAN.train()
        _freeze_gc_once(self)
        dev = self.device
        zero = lambda: torch.zeros((), device=dev)
        total_disc_loss, total_gen_loss, total_rec_loss, total_hist_loss, total_var_loss = (zero() for _ in range(5))
        gp_val, q_val = zero(), zero()
        batch_size = self.batch_size
        image_size = GAN.G.image_size
        Disc = GAN.D
        acc = self.gradient_accumulate_every
        apply_gradient_penalty = self.steps % 4 == 0

        def g_forward():
            """batch, noise and the recolouring forward of the G phase (reference :971-990)"""
            batch = next(self.loader)
            image_batch = batch['images'].to(dev)
            hist_batch = batch['histograms'].to(dev)
            noise = self.rng.image_noise(batch_size, image_size)
            return image_batch, hist_batch, self._recolor(image_batch, hist_batch, noise)

        # the G phase's forward on a second stream beside the discriminator's forward / backward (single-GPU runs; see
        # histogan_amd/trainer.py)
        overlap_g = acc == 1 and not ddp.is_dist()
        early = None

        # ---- discriminator phase (reference :927-969)
        GAN.D_opt.zero_grad()
        for i in range(acc):
            batch = next(self.loader)
            # d D(real) / d images is only needed by the gradient penalty (the reference sets requires_grad always, :897)
            image_batch = batch['images'].to(dev).detach().requires_grad_(apply_gradient_penalty)
            hist_batch = batch['histograms'].to(dev)
            noise = self.rng.image_noise(batch_size, image_size)
            with torch.no_grad():       # the reference detaches this output; no graph is needed
                generated_images = self._recolor(image_batch, hist_batch, noise)
            if overlap_g:
                early = self._side.launch(g_forward)    # after the forward above (it packed this step's weights)
            real_output, divergence, quantize_loss = discriminator_phase(
                Disc, generated_images, image_batch, batch_size,
                apply_gradient_penalty or any(q is not None for q in Disc.quantize_blocks))
            q_val = quantize_loss.detach()
            disc_loss = divergence + quantize_loss
            if apply_gradient_penalty:
                gp = gradient_penalty(image_batch, real_output)
                gp_val = gp.detach()
                disc_loss = disc_loss + gp
            disc_loss = disc_loss / acc
            disc_loss.backward()
            total_disc_loss += divergence.detach() / acc
        GAN._reduce_d.start()

        # ---- generator phase (reference :971-1048)
        GAN.G_opt.zero_grad()
        set_requires_grad(Disc, False)
        for i in range(acc):
            image_batch, hist_batch, generated_images = self._side.join(early) if early is not None else g_forward()
            early = None
            if i == 0:                  # D is updated before it scores the new fakes (reference order)
                GAN._reduce_d.finish()
                GAN.D_opt.step()
            fake_output, _ = Disc(generated_images)
            d_loss = gamma * fake_output.mean()
            generated_histograms = self.histBlock(generated_images, pre_relu=True)   # == histBlock(F.relu(.)), reference :955
            histogram_loss = hellinger_loss(hist_batch, generated_histograms, alpha)
            rec_loss = beta * self.rec_loss_func.compute_loss(image_batch, generated_images)
            gen_loss = d_loss + histogram_loss + rec_loss
            if self.variance_loss is True:
                with torch.no_grad():   # the histogram of the target histogram "image" (:1023) is data
                    input_histograms = self.histBlock_input(F.relu(hist_batch))
                    hist_gap = torch.sum(torch.abs(hist_batch - input_histograms))
                    input_gauss = gaussian_op(image_batch, kernel=self.gaussKernel)
                    input_spread = torch.std(torch.std(input_gauss, dim=2), dim=2)
                generated_gauss = gaussian_op(generated_images, kernel=self.gaussKernel)
                var_loss = -1 * (beta / 10) * hist_gap * torch.mean(torch.abs(
                    input_spread - torch.std(torch.std(generated_gauss, dim=2), dim=2)))
                gen_loss = gen_loss + var_loss
                total_var_loss += var_loss.detach() / acc
            gen_loss = gen_loss / acc
            gen_loss.backward()
            total_rec_loss += rec_loss.detach() / acc
            total_gen_loss += d_loss.detach() / acc
            total_hist_loss += histogram_loss.detach() / acc
        set_requires_grad(Disc, True)
        GAN._reduce_g()
        GAN.G_opt.step()

        # ---- one read-back per step
        stats = torch.stack([total_disc_loss, total_gen_loss, total_rec_loss, total_hist_loss, total_var_loss,
                             gp_val.reshape(()), q_val.reshape(())]).double()
        if ddp.is_dist():
            nan_flag = torch.isnan(stats[:2]).any().double().reshape(1)
            packed = torch.cat([stats, nan_flag])
            torch.distributed.all_reduce(packed[:7], op=torch.distributed.ReduceOp.SUM)
            torch.distributed.all_reduce(packed[7:], op=torch.distributed.ReduceOp.MAX)
            packed[:7] /= ddp.world_size()
            host = packed.cpu().numpy()
            has_nan = host[7] > 0 or np.isnan(host[:2]).any()
        else:
            host = stats.cpu().numpy()
            has_nan = bool(np.isnan(host[:2]).any())
        self.d_loss, self.g_loss, self.r_loss, self.h_loss = (float(v) for v in host[:4])
        if self.variance_loss is True:
            self.var_loss = float(host[4])
        if apply_gradient_penalty:
            self.last_gp_loss = float(host[5])
        self.q_loss = float(host[6])

        checkpoint_num = floor(self.steps / self.save_every)
        if has_nan:
            print(f'NaN detected for generator or discriminator. Loading from checkpoint #{checkpoint_num}')
            self.load(checkpoint_num)
            raise NanException
        if self.run_save and self.steps % self.save_every == 0:
            self.save(checkpoint_num)
        if self.run_evaluate and (self.steps % 1000 == 0 or (self.steps % 100 == 0 and self.steps < 2500)):
            self.evaluate(floor(self.steps / 1000))
        self.steps += 1
        self.av = None

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate(self, num=0, image_batch=None, hist_batch=None, triple_hist=False, double_hist=False, resizing=None,
                 resizing_method=None, swapping_levels=1, pyramid_levels=5, level_blending=False, original_size=None,
                 input_image_name=None, original_image=None, post_recoloring=False, save_input=True):
        """Recolour a batch with its target histograms and write `<num>-generated.jpg` [+ `<num>-input.jpg`]: the
        reference's parameter list (ReHistoGAN/rehistoGAN.py:1076-1081).  Post-processing as in :1130-1165:
        `resizing='downscaling'` resizes the written file to `original_size`; `resizing='upscaling'` with
        `resizing_method='pyramid'` carries the result back to the full-resolution photo `input_image_name` with the
        Laplacian-pyramid swap (`pyramid_levels`, `swapping_levels`, `level_blending`; histogan_amd/post.py) and writes
        it at the photo's size padded up to multiples of 2**pyramid_levels, as the reference does; `post_recoloring`
        then maps `original_image` (the photo, (H, W, 3) in [0, 1]) onto the colours of the unclamped network output
        with the Monge-Kantorovich transfer and overwrites the same file at the photo's size.  Both need a batch of
        one (ValueError otherwise).  `post_recoloring='idt'` does the same with the iterative distribution transfer
        (post.color_transfer_idt: nonlinear, matches the output's whole colour distribution rather than its mean and
        covariance), and `post_recoloring='palette'` with the palette transfer (post.paired_palette of the 256x256 input
        and the network output, k = 8, gives the source and destination colours with no correspondence problem;
        post.color_transfer_palette moves every pixel of the photo by a smooth blend of the per-cluster shifts), and
        `post_recoloring='lut'` with a 3D colour LUT (post.lut_fit of the 256x256 input and the network output at n = 33,
        post.lut_apply on the photo: the general smooth pointwise colour map, and the cheapest of the four to apply; a caller
        who wants the .cube file calls post.save_cube on their own post.lut_fit), and `post_recoloring='lut_refine'` with that
        LUT refined against the call's own target histogram before it is applied (post.lut_refine with the trainer's
        histogram block and its defaults: a few dozen Adam steps on the Hellinger loss the network was trained on, at the
        block's working size whatever the photo's), and `post_recoloring='idt_regrain'` with
        the distribution transfer followed by its regrain step (post.regrain(photo, post.color_transfer_idt(photo, output)):
        the colours of 'idt' on the gradient field of the photo, without the grain 'idt' leaves on flat regions); any other
        string raises ValueError, and True keeps meaning the Monge-Kantorovich map.
        `resizing_method='BGU_native'` carries the result back with bilateral guided upsampling instead (post.bgu_upsampling: the arithmetic of the reference's upsampling/BGU.m on the network's
        8-bit output, without the JPEG round trip) and writes it at exactly the photo's size.
        `resizing_method='BGU'`, which in the reference runs an external Windows executable, raises
        NotImplementedError."""
        upscale = resizing == 'upscaling'
        if isinstance(post_recoloring, str) and post_recoloring not in ('idt', 'palette', 'lut', 'idt_regrain', 'lut_refine'):
            raise ValueError(f"recoloringTrainer.evaluate: post_recoloring={post_recoloring!r} (True: the Monge-Kantorovich "
                             "linear transfer; 'idt': the iterative distribution transfer; 'palette': the palette transfer; "
                             "'lut': a fitted 3D colour LUT; 'idt_regrain': 'idt' followed by regrain; 'lut_refine': 'lut' refined against the "
                             "target histogram)")
        recolor = post_recoloring if isinstance(post_recoloring, str) else post_recoloring is True
        if upscale and resizing_method not in ('pyramid', 'BGU_native'):
            raise NotImplementedError(f"recoloringTrainer.evaluate: resizing_method={resizing_method!r} for 'upscaling' "
                                      "(implemented: 'pyramid' and 'BGU_native'; 'BGU' runs an external executable in "
                                      "the reference -- its arithmetic is available here as 'BGU_native')")
        self.GAN.eval()
        if hist_batch is None or image_batch is None:
            batch = next(self.loader_evaluate)
            image_batch = batch['images'].to(self.device)
            hist_batch = batch['histograms'].to(self.device)
            img_bt_sz = image_batch.shape[0]
            extra = ['histograms2', 'histograms3'] if triple_hist is True else (['histograms2'] if double_hist is True else [])
            if extra:               # the same images against two / three target histograms (:1089-1100)
                image_batch = torch.cat([image_batch] * (len(extra) + 1), dim=0)
                hist_batch = torch.cat([hist_batch] + [batch[k].to(self.device) for k in extra], dim=0)
        else:
            img_bt_sz = image_batch.shape[0]
        noise = self.rng.image_noise(hist_batch.shape[0], image_batch.shape[-1])
        generated_images = self._recolor(image_batch, hist_batch, noise)
        if (upscale or recolor) and generated_images.shape[0] != 1:
            raise ValueError('recoloringTrainer.evaluate: upscaling / post_recoloring need a batch of one image, got '
                             f'{generated_images.shape[0]}')
        if num is not None and self.is_main:
            from .data import save_image_grid
            ext = 'jpg' if not self.transparent else 'png'
            multi = double_hist is True or triple_hist is True
            num_rows = img_bt_sz if multi else int(np.ceil(np.sqrt(hist_batch.shape[0])))
            output_name = str(self.results_dir / self.name / f'{str(num)}-generated.{ext}')
            save_image_grid(generated_images, output_name, nrow=num_rows)
            if resizing == 'downscaling' and original_size is not None:
                from PIL import Image
                Image.open(output_name).resize((original_size[0], original_size[1])).save(output_name)
            if upscale or recolor:
                self._full_resolution(generated_images, output_name, upscale, pyramid_levels, swapping_levels,
                                      level_blending, input_image_name, original_image, recolor,
                                      resizing_method, image_batch, hist_batch)
            if save_input is True:
                save_image_grid(image_batch[:img_bt_sz] if multi else image_batch,
                                str(self.results_dir / self.name / f'{str(num)}-input.{ext}'),
                                nrow=img_bt_sz if multi else num_rows)
        return generated_images

    def _full_resolution(self, generated_images, output_name, upscale, levels, swapping_levels, blending,
                         input_image_name, original_image, recolor, method='pyramid', image_batch=None, hist_batch=None):
        """The 'upscaling' ('pyramid' or 'BGU_native') and post_recoloring branches of evaluate
        (ReHistoGAN/rehistoGAN.py:1142-1165) on the kernels of include/hg_post.h; each writes one uint8 image through
        post.save_rgb."""
        from PIL import Image
        from . import post
        if upscale:
            with Image.open(input_image_name) as im:
                ref = torch.from_numpy(np.array(im)).to(self.device)
            if method == 'BGU_native':
                post.save_rgb(post.bgu_upsampling(generated_images, ref, quantize=True), output_name)
            else:
                out = post.pyramid_upsampling(generated_images, ref, levels=levels, swapping_levels=swapping_levels,
                                              blending=blending)
                post.save_rgb(post.float_to_u8_hwc(out[0]), output_name)
        if recolor:
            if original_image is None:
                raise ValueError('recoloringTrainer.evaluate: post_recoloring needs original_image')
            src = torch.from_numpy(np.ascontiguousarray(original_image, dtype=np.float32)).to(self.device)
            if recolor == 'palette':
                pal_src, pal_dst = post.paired_palette(image_batch[0], generated_images[0], k=8)
                out, _ = post.color_transfer_palette(src, pal_src, pal_dst, quantize=True)
            elif recolor in ('lut', 'lut_refine'):
                lut = post.lut_fit(image_batch[0].permute(1, 2, 0), generated_images[0].permute(1, 2, 0), n=33)
                if recolor == 'lut_refine':
                    lut = post.lut_refine(lut, src, hist_batch, self.histBlock)
                out = post.lut_apply(src, lut, quantize=True)
            elif recolor == 'idt_regrain':
                moved, _ = post.color_transfer_idt(src, generated_images[0].permute(1, 2, 0))
                out = post.regrain(src, moved, quantize=True)
            else:
                transfer = post.color_transfer_idt if recolor == 'idt' else post.color_transfer_mkl
                out, _ = transfer(src, generated_images[0].permute(1, 2, 0), quantize=True)
            post.save_rgb(out, output_name)

    def print_log(self):
        if not self.is_main:
            return
        msg = (f'\nG: {self.g_loss:.2f} | D: {self.d_loss:.2f} | GP: {self.last_gp_loss:.2f} | R: '
               f'{self.r_loss:.2f} | H: {self.h_loss:.2f}')
        if self.variance_loss is True:
            msg += f' | V: {self.var_loss:.2f}'
        print(msg + f' | Q: {self.q_loss:.2f}')

    def save(self, num):
        if self.is_main:
            torch.save(self.GAN.state_dict(), self.model_name(num))
            self.write_config()

    def load(self, num=-1):
        self.load_config()
        name = num
        if num == -1:
            file_paths = [p for p in Path(self.models_dir / self.name).glob('model_*.pt')]
            saved_nums = sorted(map(lambda x: int(x.stem.split('_')[1]), file_paths))
            if len(saved_nums) == 0:
                return -1          # reference ReHistoGAN/rehistoGAN.py:1218: the CLI copies the pretrained HistoGAN head only then
            name = saved_nums[-1]
            print(f'continuing from previous epoch - {name}')
        self.steps = name * self.save_every
        self.GAN.load_state_dict(torch.load(self.model_name(name), map_location=self.device))
        weights_changed()
        return 0

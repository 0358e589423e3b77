"""Host-side glue added in round 3 that is plain torch (runs on the CPU): the chunked skinny GEMM, the two-copy batch
concatenation and the batched mapping-network call.  The CUDA-only branches are covered by the -m gpu network tests."""
import pytest
import torch

from histogan_amd import ops
from histogan_amd import trainer as T


@pytest.mark.parametrize('B,R,C', [(32, 2048, 1024), (2, 1024, 2048), (4, 512, 64), (3, 300, 7), (5, 12288, 96), (1, 8192, 1)])
@pytest.mark.parametrize('transposed', [True, False])
def test_skinny_mm_equals_mm(B, R, C, transposed):
    g = torch.Generator().manual_seed(B + R + C)
    a = torch.randn(B, R, generator=g, dtype=torch.float64)
    m = torch.randn(C, R, generator=g, dtype=torch.float64) if transposed else torch.randn(R, C, generator=g, dtype=torch.float64)
    ref = a @ (m.t() if transposed else m)
    out = ops._skinny_mm(a, m, transposed)
    assert out.shape == ref.shape
    assert float((out - ref).abs().max()) <= 1e-11 * max(1.0, float(ref.abs().max()))
    # gradients flow through the chunked form like through mm
    a2, m2 = a.clone().requires_grad_(True), m.clone().requires_grad_(True)
    ops._skinny_mm(a2, m2, transposed).square().sum().backward()
    a3, m3 = a.clone().requires_grad_(True), m.clone().requires_grad_(True)
    (a3 @ (m3.t() if transposed else m3)).square().sum().backward()
    assert torch.allclose(a2.grad, a3.grad, rtol=1e-10, atol=1e-10) and torch.allclose(m2.grad, m3.grad, rtol=1e-10, atol=1e-10)


def test_skinny_mm_falls_back(monkeypatch):
    a, m = torch.randn(4, 2048), torch.randn(2048, 8)
    calls = []
    real_bmm = torch.bmm
    monkeypatch.setattr(torch, 'bmm', lambda *x: calls.append(1) or real_bmm(*x))
    ops._skinny_mm(a, m, False)
    assert calls                                   # chunked
    calls.clear()
    ops._skinny_mm(a[:, ::2], m[::2], False)       # non-contiguous operands: plain mm
    ops._skinny_mm(torch.randn(4, 300), torch.randn(300, 8), False)    # reduction too short / not divisible
    monkeypatch.setattr(ops, 'SKINNY_SPLIT', False)
    ops._skinny_mm(a, m, False)
    assert not calls


def test_cat_batches_equals_cat():
    a, b = torch.randn(3, 3, 8, 8), torch.randn(5, 3, 8, 8)
    assert torch.equal(T._cat_batches(a, b), torch.cat((a, b), 0))
    br = b.clone().requires_grad_(True)
    out = T._cat_batches(a, br)                    # a graph is needed: falls back to torch.cat
    assert out.requires_grad and torch.equal(out.detach(), torch.cat((a, b), 0))
    assert torch.equal(T._cat_batches(a, b.double()).double(), torch.cat((a.double(), b.double()), 0))   # dtype mismatch: cat's rules


def test_latent_to_w_layer_counts_and_fallback():
    S = torch.nn.Sequential(torch.nn.Linear(16, 16), torch.nn.LeakyReLU(0.2))
    z1, z2 = torch.randn(4, 16), torch.randn(4, 16)
    out = T.latent_to_w(S, [(z1, 3), (z2, 2)])
    assert [n for _, n in out] == [3, 2]
    assert torch.equal(out[0][0], S(z1)) and torch.equal(out[1][0], S(z2))
    t = T.styles_def_to_tensor(out)
    assert t.shape == (4, 5, 16) and torch.equal(t[:, 2], out[0][0]) and torch.equal(t[:, 3], out[1][0])


def test_demod_backward_formulas_equal_autograd_of_the_reference_expression():
    """The closed forms hg_demod_weight_term / hg_demod_style_grad implement (and the GPU tests compare the kernels with) are
    the gradients of the reference's demodulation, histoGAN/histoGAN.py:427-429, written there on per-sample weights:
        weights = w[None] * (y[:, None, :, None, None] + 1);  d = rsqrt((weights ** 2).sum(dim=(2, 3, 4)) + EPS)
    Checked here against autograd of exactly that expression in fp64."""
    g = torch.Generator().manual_seed(5)
    B, N, K, k = 3, 6, 5, 3
    w = torch.randn(N, K, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randn(B, K, generator=g, dtype=torch.float64, requires_grad=True)
    gd = torch.randn(B, N, generator=g, dtype=torch.float64)
    weights = w[None] * (y[:, None, :, None, None] + 1)
    d = torch.rsqrt((weights ** 2).sum(dim=(2, 3, 4)) + 1e-8)
    gy_ref, gw_ref = torch.autograd.grad(d, (y, w), gd)
    with torch.no_grad():
        s1 = y + 1
        wsq = w.pow(2).sum(dim=(2, 3))
        assert torch.allclose(torch.rsqrt((s1 * s1) @ wsq.t() + 1e-8), d, rtol=1e-12, atol=0)      # the shared-weight form of d
        gq = gd * (-0.5) * d ** 3
        gy = 2.0 * s1 * (gq @ wsq)                                   # hg_demod_style_grad
        gw = 2.0 * w * (gq.t() @ (s1 * s1))[:, :, None, None]        # hg_demod_weight_term
    assert torch.allclose(gy, gy_ref, rtol=1e-10, atol=1e-12) and torch.allclose(gw, gw_ref, rtol=1e-10, atol=1e-12)


def test_environment_switches_of_the_python_layer_are_the_documented_ones():
    """Every HG_* variable histogan_amd/*.py reads from the environment is a row of the first table under 'Environment
    switches' in DESIGN.md, and the other way round.  The sources are read as text (nothing is imported), so an A/B switch
    added for an experiment shows up here until it is documented or retired."""
    import pathlib
    import re
    root = pathlib.Path(__file__).resolve().parents[1]
    read = set()
    for src in sorted((root / 'histogan_amd').glob('*.py')):
        read |= set(re.findall(r"""os\.environ\.get\(\s*['"](HG_[A-Z0-9_]+)['"]""", src.read_text()))
    lines = (root / 'DESIGN.md').read_text().split('\n')
    at = lines.index('### Environment switches')
    first = next(i for i in range(at, len(lines)) if lines[i].startswith('|'))
    documented = set()
    for line in lines[first + 2:]:                   # rows of the first table (behind its header and separator)
        if not line.startswith('|'):
            break
        documented |= set(re.findall(r'`(HG_[A-Z0-9_]+)`', line.split('|')[1]))
    assert read and read == documented, (sorted(read - documented), sorted(documented - read))


def test_switches_of_the_hip_sources_are_the_documented_ones():
    """Every getenv("HG_...") name and every HG_... name a preprocessor conditional tests (#if, #ifdef, #ifndef, #elif:
    with or without a default block) in histogan_amd/csrc/ is a row of the table under 'Launcher knobs and build flags' in
    DESIGN.md, and the other way round.  The sources are read as text, so a knob added for an experiment shows up here
    until it is documented or retired."""
    import pathlib
    import re
    root = pathlib.Path(__file__).resolve().parents[1]
    read = set()
    for src in sorted(p for p in (root / 'histogan_amd' / 'csrc').iterdir() if p.suffix in ('.hip', '.h')):
        text = src.read_text()
        read |= set(re.findall(r'getenv\(\s*"(HG_[A-Z0-9_]+)"', text))
        for cond in re.findall(r'^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$', text, re.M):
            read |= set(re.findall(r'\bHG_[A-Z0-9_]+\b', cond))
    lines = (root / 'DESIGN.md').read_text().split('\n')
    at = lines.index('### Launcher knobs and build flags')
    first = next(i for i in range(at, len(lines)) if lines[i].startswith('|'))
    documented = set()
    for line in lines[first + 2:]:                   # rows of the table (behind its header and separator)
        if not line.startswith('|'):
            break
        documented |= set(re.findall(r'`(HG_[A-Z0-9_]+)`', line.split('|')[1]))
    assert read and read == documented, (sorted(read - documented), sorted(documented - read))


def test_launch_layer_has_one_place_per_kernel_and_per_helper():
    """The binding layer's structure, read from the sources: every generator kernel of include/hg_nets.h that ops.py and gfused.py
    share is marshalled in exactly one place (launch.py), the small host helpers exist once (in _lib.py), and ops.py / conv.py
    do not import each other behind a function.  Then the helpers' own contract, on CPU tensors."""
    import ast
    import pathlib
    import re
    pkg = pathlib.Path(__file__).resolve().parents[1] / 'histogan_amd'
    src = {p.name: p.read_text() for p in sorted(pkg.glob('*.py'))}
    tree = {name: ast.parse(text) for name, text in src.items()}

    def calls(fn):           # name of module -> number of `lib.<fn>(` call sites in it
        return {name: len(re.findall(r'\blib\.' + fn + r'\(', text)) for name, text in src.items()
                if re.search(r'\blib\.' + fn + r'\(', text)}

    for fn in ('hg_modulate_fwd', 'hg_modulate_bwd', 'hg_demod_noise_lrelu_fwd', 'hg_demod_noise_lrelu_bwd', 'hg_torgb_fwd',
               'hg_torgb_bwd', 'hg_demod_style_grad', 'hg_channel_sum'):
        assert calls(fn) == {'launch.py': 1}, (fn, calls(fn))
    assert set(calls('hg_nets_workspace_bytes').values()) == {1}, calls('hg_nets_workspace_bytes')     # one per wrapper module
    assert not any(re.search(r'48\s*\*\s*1024', src[name]) for name in ('ops.py', 'gfused.py'))    # the to-RGB LDS limit: launch.py's

    helpers = {'stream_of', 'f32c', 'ptr', 'need_gpu', 'workspace', 'NullCtx',                      # _lib's
               '_st', '_stream', '_f32c', '_ptr', '_need_gpu', '_need_cuda', '_require_gpu', '_NullCtx'}   # the former copies
    lib_defs = {n.name for n in tree['_lib.py'].body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    assert helpers & lib_defs == {'stream_of', 'f32c', 'ptr', 'need_gpu', 'workspace', 'NullCtx'}
    for name, t in tree.items():
        if name == '_lib.py':
            continue
        defs = {n.name for n in ast.walk(t) if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
        assert not defs & helpers, (name, sorted(defs & helpers))
        assert not re.search(r'torch\.empty\(\(?max\(\w+, 4\)', src[name]), name     # the workspace pattern written out

    def imports(node):       # module names an import statement reaches, relative ones without their dots
        if isinstance(node, ast.Import):
            return {a.name for a in node.names}
        if isinstance(node, ast.ImportFrom):
            return {node.module} if node.module else {a.name for a in node.names}
        return set()

    for name, other in (('ops.py', 'conv'), ('conv.py', 'ops')):
        top = set(tree[name].body)
        inner = [n for n in ast.walk(tree[name]) if n not in top and other in imports(n)]
        assert not inner, (name, [n.lineno for n in inner])
    assert not any('ops' in imports(n) for n in ast.walk(tree['conv.py']))        # conv sits below ops
    for n in ast.walk(tree['launch.py']):                                        # and launch below both: _lib and torch only
        assert imports(n) <= {'torch', '_lib'}, (n.lineno, imports(n))
    assert not any(isinstance(n, ast.ImportFrom) and n.module == 'ops' and any(a.name.startswith('_') for a in n.names)
                   for n in ast.walk(tree['reops.py']))

    from histogan_amd._lib import f32c, ptr
    a = torch.randn(3, 4, requires_grad=True)
    b = f32c(a)
    assert b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr() and not b.requires_grad and b.shape == a.shape
    c = f32c(torch.arange(6, dtype=torch.float64).reshape(2, 3))
    assert c.dtype == torch.float32 and torch.equal(c, torch.arange(6.).reshape(2, 3))
    s = torch.randn(4, 6)[:, ::2]
    e = f32c(s)
    assert not s.is_contiguous() and e.is_contiguous() and torch.equal(e, s)
    assert ptr(None) is None and ptr(a) == a.data_ptr()

"""B1 drop-in claim: after ``rewriting_amd.install_reference_aliases()`` the reference's own
drivers and UI import this package under the reference's module names, and the reference's modules this package
does not rebuild keep coming from the reference checkout.

Running the reference's drivers themselves on this package (``metrics/make_watermark_images.py`` main(),
``metrics/sample_edited.py``) needs a checkout of the reference: ``python tests/dropin_driver.py --mode ours --out X``
does it, and tests/golden/dropin/ holds the PNGs the same drivers write on the reference itself."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_aliases_keep_the_reference_ui_modules_importable(tmp_path):
    """rewrite/rewriteapp.py does `from utils import ... show, labwidget, paintwidget, imgviz`: those modules are
    not rebuilt here and must still come from the reference checkout, next to this package's nethook / renormalize --
    and the checkout's own files of the modules this package does rebuild never shadow them.  The checkout is a
    stand-in written here: one file per module name, each recording where it came from."""
    ref_root = tmp_path / 'reference'
    (ref_root / 'utils' / 'stylegan2').mkdir(parents=True)
    (ref_root / 'rewrite').mkdir()
    for name in ('show', 'labwidget', 'paintwidget', 'pidfile', 'imgsave'):
        (ref_root / 'utils' / (name + '.py')).write_text('ORIGIN = "reference"\n')
    for name in ('utils/nethook', 'utils/renormalize', 'utils/pbar', 'utils/tally', 'utils/zdataset',
                 'utils/stylegan2/models', 'rewrite/ganrewrite'):
        (ref_root / (name + '.py')).write_text('raise ImportError("the reference copy of %s was imported")\n' % name)
    code = (
        "import sys, types; sys.path.insert(0, %r)\n"
        "tv = types.ModuleType('torchvision'); tr = types.ModuleType('torchvision.transforms')\n"
        "fn = types.ModuleType('torchvision.transforms.functional'); tr.functional = fn; tv.transforms = tr\n"
        "tv.models = types.ModuleType('torchvision.models')\n"
        "sys.modules.update({'torchvision': tv, 'torchvision.transforms': tr, 'torchvision.transforms.functional': fn,"
        " 'torchvision.models': tv.models})\n"
        "import rewriting_amd; rewriting_amd.install_reference_aliases(reference_root=%r)\n"
        "from utils import nethook, renormalize, pbar, tally, zdataset, labwidget, paintwidget, pidfile, imgsave\n"
        "import utils.stylegan2.models as m, rewrite.ganrewrite as g\n"
        "assert nethook.__name__ == 'rewriting_amd.utils.nethook' and g.__name__ == 'rewriting_amd.rewrite.ganrewrite'\n"
        "assert m.__name__ == 'rewriting_amd.utils.stylegan2.models'\n"
        "assert labwidget.__file__.startswith(%r) and pidfile.__file__.startswith(%r)\n"
        "assert labwidget.ORIGIN == pidfile.ORIGIN == 'reference'\n"
        "print('ok')\n" % (ROOT, str(ref_root), str(ref_root), str(ref_root)))
    proc = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0 and proc.stdout.strip().endswith('ok'), proc.stdout + proc.stderr[-3000:]

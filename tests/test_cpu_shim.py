"""The ``ava/`` shim of this repo overrides ONLY ``ava.models.vae``: with the repo ahead of the reference on
``sys.path`` (method 1) every other ``ava.*`` import of the example scripts
(``examples/mouse_sylls_mwe.py:20-30``) still resolves to the reference package.  Runs in a subprocess so that the
path order of this test session does not matter.

The reference package is stood in for by a tree written into a temporary directory: the module paths the example
imports, each defining the names it imports, ``ava/__init__.py`` with the reference's ``__version__``, the
reference's ``from ava.models.vae import VAE`` in ``ava/data/data_container.py`` (data_container.py:33) and an
``ava/models/vae.py`` that fails on import, so that the shim's module must be the one that loads."""
import os
import subprocess
import sys
import textwrap

from conftest import ROOT

# module path -> source of the stand-in reference package
UPSTREAM = {
    "ava/__init__.py": '__version__ = "0.3.1"\n',
    "ava/data/__init__.py": "",
    "ava/data/data_container.py": "from ava.models.vae import VAE\n\n\nclass DataContainer:\n    pass\n",
    "ava/models/__init__.py": "",
    "ava/models/vae.py": 'raise ImportError("the reference\'s own ava.models.vae was imported: the shim does not override it")\n',
    "ava/models/vae_dataset.py": "def get_syllable_partition(*a, **k):\n    pass\n\n\n"
                                 "def get_syllable_data_loaders(*a, **k):\n    pass\n",
    "ava/preprocessing/__init__.py": "",
    "ava/preprocessing/preprocess.py": "def process_sylls(*a, **k):\n    pass\n\n\n"
                                       "def tune_syll_preprocessing_params(*a, **k):\n    pass\n",
    "ava/preprocessing/utils.py": "def get_spec(*a, **k):\n    pass\n",
    "ava/segmenting/__init__.py": "",
    "ava/segmenting/refine_segments.py": "def refine_segments_pre_vae(*a, **k):\n    pass\n",
    "ava/segmenting/segment.py": "def tune_segmenting_params(*a, **k):\n    pass\n\n\ndef segment(*a, **k):\n    pass\n",
    "ava/segmenting/amplitude_segmentation.py": "def get_onsets_offsets(*a, **k):\n    pass\n",
    "ava/plotting/__init__.py": "",
    "ava/plotting/tooltip_plot.py": "def tooltip_plot_DC(*a, **k):\n    pass\n",
    "ava/plotting/latent_projection.py": "def latent_projection_plot_DC(*a, **k):\n    pass\n",
}


def _upstream(tmp_path):
    ref = tmp_path / "reference"
    for rel, src in UPSTREAM.items():
        path = ref / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(src)
    return str(ref)


def _run(code, paths, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join(paths)
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout


def test_shim_alone_provides_the_vae_module(tmp_path):
    out = _run("from ava.models.vae import X_SHAPE, X_DIM, VAE\n"
               "import ava\n"
               "print(VAE.__module__, X_SHAPE, X_DIM, ava.__version__)", [ROOT], str(tmp_path))
    assert out.split()[0] == "ava_amd.vae" and "(128, 128) 16384" in out


def test_shim_overrides_only_ava_models_vae(tmp_path):
    ref = _upstream(tmp_path)
    # the import block of examples/mouse_sylls_mwe.py:20-30, verbatim module paths
    code = textwrap.dedent('''
        from ava.data.data_container import DataContainer
        from ava.models.vae import X_SHAPE, VAE
        from ava.models.vae_dataset import get_syllable_partition, get_syllable_data_loaders
        from ava.preprocessing.preprocess import process_sylls, tune_syll_preprocessing_params
        from ava.preprocessing.utils import get_spec
        from ava.segmenting.refine_segments import refine_segments_pre_vae
        from ava.segmenting.segment import tune_segmenting_params, segment
        from ava.segmenting.amplitude_segmentation import get_onsets_offsets
        from ava.plotting.tooltip_plot import tooltip_plot_DC
        from ava.plotting.latent_projection import latent_projection_plot_DC
        import ava, ava.models.vae, ava.models.vae_dataset, ava.data.data_container as dc
        print(VAE.__module__)
        print(ava.models.vae.__file__)
        print(ava.models.vae_dataset.__file__)
        print(dc.__file__)
        print(dc.VAE.__module__)          # DataContainer._make_latent_means (data_container.py:458-475) builds THIS class
        print(ava.__version__)
    ''')
    out = _run(code, [ROOT, ref], str(tmp_path)).split("\n")
    assert out[0] == "ava_amd.vae"
    assert out[1] == os.path.join(ROOT, "ava", "models", "vae.py")
    assert out[2].startswith(ref) and out[3].startswith(ref)
    assert out[4] == "ava_amd.vae"
    assert out[5] == "0.3.1"

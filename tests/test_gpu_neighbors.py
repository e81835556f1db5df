"""The shotgun-movie search on the MI355X (row f7): ava_amd.neighbors against sklearn / the reference's latent_nn loop
(tests/golden/neighbors.npz) and an fp64 numpy restatement, the tie and NaN rules, chunking and reproducibility, and
ava_amd.shotgun_movie end to end."""
import os

import numpy as np
import pytest
import torch

import neighbor_cases as NC
from conftest import load_golden
from ava_amd import neighbors as N, shotgun_movie as SM, synthetic as syn
from ava_amd.spec import DeviceAudio, get_spec_batch

pytestmark = pytest.mark.gpu


def _check_against(idx, dist, want_dist, want_gap, D, metric):
    """distances within 1e-12 (absolute for correlation, relative for euclidean); indices equal where the best is
    clear by more than 1e-9, elsewhere the pick is within 1e-12 of the minimum"""
    if metric == "correlation":
        np.testing.assert_allclose(dist, want_dist, rtol=0, atol=1e-12)
    else:
        np.testing.assert_allclose(dist, want_dist, rtol=1e-12, atol=0)
    clear = want_gap > 1e-9
    ref_idx, ref_dist = NC.nearest_from_distances(D, metric)
    np.testing.assert_array_equal(idx[clear], ref_idx[clear])
    picked = D[np.arange(len(D)), idx]
    np.testing.assert_allclose(picked, ref_dist, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", sorted(NC.CASES))
def test_golden_case(name):
    golden = load_golden("neighbors.npz")
    metric = NC.CASES[name][0]
    q, r = NC.case_inputs(name)
    idx, dist = N.nearest(q, r, metric=metric)
    assert idx.dtype == np.int64 and dist.dtype == np.float64 and idx.shape == (len(q),)
    D = NC.distances(q, r, metric)
    _check_against(idx, dist, golden[name + "_dist"], golden[name + "_gap"], D, metric)
    clear = golden[name + "_gap"] > 1e-9
    np.testing.assert_array_equal(idx[clear], golden[name + "_idx"][clear])
    # device tensors in, same answer bit for bit
    idx2, dist2 = N.nearest(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), metric=metric)
    np.testing.assert_array_equal(idx2, idx)
    np.testing.assert_array_equal(dist2, dist)


@pytest.mark.parametrize("metric", ["correlation", "euclidean"])
@pytest.mark.parametrize("chunk_rows", [None, 2])
def test_duplicates_resolve_to_lowest_index(metric, chunk_rows):
    r = NC.make_inputs(metric, 1, 300, 40, "float64", 610)[1]
    r[[7, 150, 299]] = r[5]
    q = np.stack([r[5] + 1e-3 * np.cos(np.arange(40)), r[5]])
    idx, dist = N.nearest(q, r, metric=metric, chunk_rows=chunk_rows)
    np.testing.assert_array_equal(idx, [5, 5])
    same = np.repeat(r[:1], 200, axis=0)                       # every reference equal: index 0 everywhere
    idx, _ = N.nearest(q, same, metric=metric, chunk_rows=chunk_rows)
    np.testing.assert_array_equal(idx, [0, 0])


@pytest.mark.parametrize("chunk_rows", [None, 3])
def test_correlation_nan_rules(chunk_rows):
    d = 50
    ramp = np.arange(d, dtype=np.float64)
    r = np.full((260, d), 0.75)                                # zero variance: NaN distances
    r[200] = -ramp                                             # the only real candidate, distance 2
    q = np.stack([ramp, np.full(d, 3.0)])                      # the second query has zero variance itself
    idx, dist = N.nearest(q, r, chunk_rows=chunk_rows)
    assert idx[0] == 200 and abs(dist[0] - 2.0) < 1e-12
    assert idx[1] == 0 and np.isnan(dist[1])
    idx, dist = N.nearest(q.astype(np.float32), np.full((70, d), 0.5, dtype=np.float32), chunk_rows=chunk_rows)
    np.testing.assert_array_equal(idx, [0, 0])
    assert np.isnan(dist).all()


@pytest.mark.parametrize("chunk_rows", [None, 4])
def test_euclidean_first_nan_wins(chunk_rows):
    rng_r = syn.gauss(100 * 8, 620).reshape(100, 8)
    q = rng_r[[2, 60]] + 0.0
    r = rng_r.copy()
    r[9, 3] = np.nan
    r[77, 0] = np.nan
    idx, dist = N.nearest(q, r, metric="euclidean", chunk_rows=chunk_rows)
    want = [np.argmin([np.sqrt(np.sum((qi - rj) ** 2)) for rj in r]) for qi in q]
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(idx, [9, 9])
    assert np.isnan(dist).all()


def test_large_correlation_chunking_and_reproducibility():
    q, r = NC.make_inputs("correlation", 300, 5000, 16384, "float32", 630, dup=1)
    idx, dist = N.nearest(q, r)
    D = NC.distances(q, r, "correlation")
    _, want_dist = NC.nearest_from_distances(D, "correlation")
    _check_against(idx, dist, want_dist, NC.gap(D), D, "correlation")
    idx_c, dist_c = N.nearest(q, r, chunk_rows=777)             # host chunks, merged on the device
    np.testing.assert_array_equal(idx_c, idx)
    np.testing.assert_array_equal(dist_c, dist)
    rd = torch.from_numpy(r).cuda()
    qd = torch.from_numpy(q).cuda()
    for _ in range(2):
        idx_d, dist_d = N.nearest(qd, rd)
        np.testing.assert_array_equal(idx_d, idx)
        np.testing.assert_array_equal(dist_d, dist)
    idx_d, dist_d = N.nearest(qd, rd, chunk_rows=777)            # device chunks
    np.testing.assert_array_equal(idx_d, idx)
    np.testing.assert_array_equal(dist_d, dist)


# ---- ava_amd.shotgun_movie end to end --------------------------------------------------------------------------------

class _DC:
    """stand-in for ava.data.data_container.DataContainer: request() and model_filename"""

    def __init__(self, model_filename, fields):
        self.model_filename = model_filename
        self.fields = fields
        self.requested = []

    def request(self, field):
        self.requested.append(field)
        return self.fields[field]


class _SimpleDataset(torch.utils.data.Dataset):
    """shotgun_movie.py:194-202"""

    def __init__(self, specs):
        self.specs = specs

    def __len__(self):
        return self.specs.shape[0]

    def __getitem__(self, index):
        return torch.from_numpy(self.specs[index]).type(torch.FloatTensor)


@pytest.fixture(scope="module")
def movie_setup(tmp_path_factory):
    from scipy.io import wavfile
    from ava_amd.vae import VAE
    tmp = tmp_path_factory.mktemp("shotgun")
    p = dict(syn.FINCH_PARAMS)
    audio = syn.recordings(n_files=1, fs=p['fs'], seconds=1.2)[0][0]
    wav = str(tmp / "song.wav")
    wavfile.write(wav, p['fs'], audio)
    model = VAE(z_dim=32, device_name="cuda")
    fp = syn.fixture_parameters(32)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            prm.copy_(torch.from_numpy(fp[name]))
    ckpt = str(tmp / "checkpoint.tar")
    model.save_state(ckpt)
    n_ref = 120
    ref_specs = syn.spectrograms(n_ref, salt=777)
    onsets = SM.window_onsets(len(audio), p['fs'], p['window_length'], 30, 0.01)
    win = SM.window_spectrograms(audio, p['fs'], onsets, p, 0.01).cpu().numpy()
    ref_specs[::12] = 0.6 * win[:len(ref_specs[::12])] + 0.4 * ref_specs[::12]     # some windows have close relatives
    fields = {'specs': ref_specs, 'latent_means': syn.gauss(n_ref * 32, 91).reshape(n_ref, 32),
              'latent_mean_umap': syn.gauss(n_ref * 2, 92).reshape(n_ref, 2)}
    return dict(p=p, audio=audio, wav=wav, ckpt=ckpt, fields=fields, tmp=tmp)


def test_window_spectrograms_equal_per_window_get_spec_batch(movie_setup):
    s = movie_setup
    p, audio = s['p'], s['audio']
    onsets = SM.window_onsets(len(audio), p['fs'], p['window_length'], 30, 0.01)
    specs = SM.window_spectrograms(audio, p['fs'], onsets, p, 0.01, chunk=7).cpu().numpy()
    assert specs.shape == (len(onsets), p['num_freq_bins'], p['num_time_bins'])
    dev_audio = DeviceAudio([audio])
    for i, onset in enumerate(onsets):
        offset = onset + p['window_length']
        one = get_spec_batch(dev_audio, [0], [onset - 0.01], [offset + 0.01], p, p['fs'],
                             np.linspace(onset, offset, p['num_time_bins'])[None, :])
        np.testing.assert_array_equal(specs[i], one[0].cpu().numpy())


def test_embedding_spectrogram_correlation(movie_setup):
    s = movie_setup
    p, audio = s['p'], s['audio']
    dc = _DC(s['ckpt'], s['fields'])
    new_embed, original_embed, indices, onsets = SM.shotgun_movie_embedding(dc, s['wav'], p)
    assert dc.requested == ['specs', 'latent_mean_umap']
    np.testing.assert_array_equal(onsets, SM.window_onsets(len(audio), p['fs'], p['window_length'], 30, 0.01))
    specs = SM.window_spectrograms(audio, p['fs'], onsets, p, 0.01).cpu().numpy().reshape(len(onsets), -1)
    D = NC.distances(specs, s['fields']['specs'].reshape(len(s['fields']['specs']), -1), "correlation")
    assert (NC.gap(D) > 1e-9).all()
    np.testing.assert_array_equal(indices, NC.nearest_from_distances(D, "correlation")[0])
    np.testing.assert_array_equal(new_embed, original_embed[indices])


def test_embedding_latent_nn(movie_setup):
    from ava_amd.vae import VAE
    s = movie_setup
    p, audio = s['p'], s['audio']
    dc = _DC(s['ckpt'], s['fields'])
    new_embed, original_embed, indices, onsets = SM.shotgun_movie_embedding(dc, s['wav'], p, method='latent_nn')
    assert dc.requested == ['latent_mean_umap', 'latent_means']
    specs = SM.window_spectrograms(audio, p['fs'], onsets, p, 0.01)
    latent = SM.window_latents(s['ckpt'], specs)
    # the reference: VAE().load_state(...); get_latent(DataLoader(SimpleDataset(specs))) -- batches of one, train mode
    model = VAE(z_dim=32)
    model.load_state(s['ckpt'])
    assert model.training
    want = model.get_latent(torch.utils.data.DataLoader(_SimpleDataset(specs.cpu().numpy())))
    np.testing.assert_array_equal(latent, want)
    D = NC.distances(latent, s['fields']['latent_means'], "euclidean")
    assert (NC.gap(D) > 1e-9).all()
    np.testing.assert_array_equal(indices, NC.nearest_from_distances(D, "euclidean")[0])
    np.testing.assert_array_equal(new_embed, original_embed[indices])


def test_shotgun_movie_dc_frames_and_ffmpeg_argv(movie_setup, monkeypatch):
    s = movie_setup
    p = s['p']
    calls = []
    real_popen = SM.subprocess.Popen

    class _Done:
        def communicate(self):
            return b"", None

    def _popen(cmd, *args, **kwargs):
        if isinstance(cmd, list) and cmd[:1] == ["ffmpeg"]:
            calls.append(list(cmd))
            return _Done()
        return real_popen(cmd, *args, **kwargs)         # anything else (matplotlib, torch) runs as usual

    monkeypatch.setattr(SM.subprocess, "Popen", _popen)
    out_dir = str(s['tmp'] / "frames")
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, "stale.jpg"), "w").close()
    SM.shotgun_movie_DC(_DC(s['ckpt'], s['fields']), s['wav'], p, output_dir=out_dir, fps=30, mp4_fn="movie.mp4")
    n = len(SM.window_onsets(len(s['audio']), p['fs'], p['window_length'], 30, 0.01))
    frames = sorted(f for f in os.listdir(out_dir) if f.endswith(".jpg"))
    assert frames == ["viz-%05d.jpg" % i for i in range(n)]
    assert calls == [["ffmpeg", "-y", "-r", "30", "-i", os.path.join(out_dir, "viz-%05d.jpg"), "temp.mp4"],
                     ["ffmpeg", "-y", "-r", "30", "-i", "temp.mp4", "-i", s['wav'], "-c:a", "aac", "-strict", "-2",
                      os.path.join(out_dir, "movie.mp4")]]

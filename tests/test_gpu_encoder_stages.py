"""The audio encoder's HIP stages one by one against plain fp64 references (tests/encoder_reference.py; pinned on the CPU by
tests/test_encoder_reference_host.py, which also holds the stock fp32 branch to half these tolerances on the same inputs):

  ddsp_loudness       every n_fft, per frame, 2e-6 absolute, no frame excluded: level steps between the two frames that share a
                      packed transform, digital silence beside noise, an overlapped onset, a NaN and an Inf sample
  ddsp_resample       ten rate pairs, lengths around one window and one polyphase period, 1e-6 absolute; a row past the grid's cap;
                      the stock-ops fallback for a pair whose table does not fit the kernel's LDS
  ddsp_crepe_frames   mean / std within one fp32 ulp of fp64; frames bit-equal to the fp32 expression from the kernel's own stats
  ddsp_pitch_decode   probabilities within 3e-7 of the fp64 sigmoid; bin, harmonicity, f0, cents consistent with torch.argmax of
                      the kernel's own probabilities, on ties, saturation, NaN and Inf rows

Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import ddsp_pytorch_amd as ddsp
from ddsp_pytorch_amd import dataset
from dataset_common import DataConf

import encoder_reference as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- loudness

@pytest.mark.parametrize("n_fft", R.LOUDNESS_SIZES)
def test_loudness_every_frame_against_fp64(n_fft):
    aw = R.a_weight_of(n_fft)
    worst = {}                                   # quiet / loud ratio of a frame to its pair partner -> worst error
    bad = []
    for c in R.loudness_cases(n_fft):
        enc = R.loudness_encoder(n_fft, c["hop"]).cuda()
        x = torch.from_numpy(c["x"]).cuda()
        y = enc(x)
        got = y.cpu().numpy()[..., 0].astype(np.float64)
        ref = R.loudness_ref(c["x"], n_fft, c["hop"], aw)
        assert got.shape == ref.shape
        dead = c["nan_frames"]
        # a frame that holds a NaN / Inf sample is NaN, and no other frame is: the pair partner stays finite
        if not np.array_equal(np.isnan(got), dead):
            bad.append((c["name"], "NaN frames", np.argwhere(np.isnan(got) != dead).tolist()))
        err = np.where(dead | np.isnan(got), 0.0, np.abs(got - ref))
        ratio = R.pair_ratio(c["levels"]) if c["levels"] is not None else np.full(err.shape, -1.0)
        for r in np.unique(ratio):
            key = c["name"] if r < 0 else float(f"{r:.3g}")
            worst[key] = max(worst.get(key, 0.0), float(err[ratio == r].max()))
        if err.max() > R.LOUDNESS_TOL:
            bad.append((c["name"], float(err.max()), np.argwhere(err > R.LOUDNESS_TOL).tolist()))
        # each row alone gives the same bits as in the batch, and so does a second call
        for b in range(x.shape[0]):
            if not np.array_equal(_bits(enc(x[b:b + 1]).cpu().numpy()[0]), _bits(y[b].cpu().numpy())):
                bad.append((c["name"], "row alone differs", b))
        if not np.array_equal(_bits(enc(x).cpu().numpy()), _bits(y.cpu().numpy())):
            bad.append((c["name"], "second call differs"))
    print(f"\nloudness n_fft {n_fft}: worst |kernel - fp64| by pair ratio / case: "
          + ", ".join(f"{k}: {v:.2e}" for k, v in sorted(worst.items(), key=lambda kv: str(kv[0]))))
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------- resampler

@pytest.mark.parametrize("orig,new", R.RATE_PAIRS)
def test_resampler_against_fp64(orig, new):
    rs = ddsp.encoder.Resample(orig, new).cuda()
    assert rs.fits_kernel
    worst, bad = {}, []
    for L in R.resample_lengths(orig, new):
        xh = R.resample_input(orig, new, L)
        x = torch.from_numpy(xh).cuda()
        y = rs(x)
        ref = R.resample_ref(xh, orig, new)
        assert tuple(y.shape) == ref.shape
        worst[L] = float(np.abs(y.cpu().numpy() - ref).max())
        if worst[L] > R.RESAMPLE_TOL:
            bad.append((L, worst[L]))
        for b in range(3):                                                   # a row of a batch equals the row alone, bitwise
            if not torch.equal(rs(x[b:b + 1])[0], y[b]):
                bad.append((L, "row alone differs", b))
    print(f"\nresample {orig} -> {new} ({rs.new} x {rs.ntaps} taps): worst |kernel - fp64| by length: {worst}")
    assert not bad, bad


def test_resampler_past_the_grid_cap():
    orig, new = R.LONG_PAIR
    xh = R.resample_input(orig, new, R.LONG_LENGTH, rows=1)
    y = ddsp.encoder.Resample(orig, new).cuda()(torch.from_numpy(xh).cuda())
    assert y.shape[1] > 16384 * 1024
    pos = R.long_positions(y.shape[1])
    got = y[:, torch.from_numpy(pos).cuda()].cpu().numpy()
    err = np.abs(got - R.resample_ref(xh, orig, new, positions=pos))
    print(f"\nresample {orig} -> {new}, {y.shape[1]} outputs: worst first / last / drawn 4096: "
          f"{err[:, :4096].max():.2e} / {err[:, 4096:8192].max():.2e} / {err[:, 8192:].max():.2e}")
    assert err.max() <= R.RESAMPLE_TOL


def test_resampler_falls_back_to_stock_ops_when_the_table_does_not_fit(tmp_path):
    from scipy.io import wavfile
    orig, new = 44056, 16000                                                 # 5507 : 2000, 2000 x 34 taps > 16384 floats
    rs = ddsp.encoder.Resample(orig, new).cuda()
    assert not rs.fits_kernel and rs.new * rs.ntaps > 16384
    xh = R.resample_input(orig, new, 6000)
    y = rs(torch.from_numpy(xh).cuda())
    ref = R.resample_ref(xh, orig, new)
    assert y.is_cuda and tuple(y.shape) == ref.shape
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f"\nresample {orig} -> {new} (stock ops on the device): worst |y - fp64| {err:.2e}")
    assert err <= R.RESAMPLE_TOL
    # the dataset's call takes the same route
    mono = R.resample_input(orig, new, 20000, rows=1)[0]
    path = str(tmp_path / "odd_rate.wav")
    wavfile.write(path, orig, mono)
    conf = DataConf(str(tmp_path), new, 1024, 256, 2, 0.25, 0.125)
    audio = dataset.DeviceAudio.from_files([path], conf, torch.device("cuda"))
    ref = R.resample_ref(mono[None], orig, new)[0]
    assert audio.y.shape == ref.shape
    assert float(np.abs(audio.y.cpu().numpy() - ref).max()) <= R.RESAMPLE_TOL


# ------------------------------------------------------------------------------------------------- row statistics and framing

def _frame_rows(Lr, seed):
    rng = np.random.default_rng([Lr, seed, 23])
    rows = [0.3 * rng.standard_normal(Lr),                          # plain noise
            100.0 + 1e-3 * rng.standard_normal(Lr),                 # the fp64 sums matter here
            -7.0 + 5.0 * rng.standard_normal(Lr),                   # another offset and scale
            np.full(Lr, 0.1),                                       # constant: std 0
            np.zeros(Lr)]                                           # silence: std 0
    return np.stack(rows).astype(np.float32)


def _crepe_frames(y, hop, T):
    B, Lr = y.shape
    stats = torch.full((B, 2), 7.0, device="cuda")
    frames = torch.full((B * T, 1532), 7.0, device="cuda")
    rc = ddsp._lib.lib().ddsp_crepe_frames(y.data_ptr(), stats.data_ptr(), frames.data_ptr(), B, Lr, hop, T, None)
    ddsp._lib.check(rc, "ddsp_crepe_frames")
    torch.cuda.synchronize()
    return stats.cpu().numpy(), frames.cpu().numpy()


FRAME_SHAPES = [(1024, 92, 1, 5), (1300, 92, 4, 5), (1301, 92, 4, 5), (1345, 92, 4, 5), (1391, 92, 4, 5), (1028, 1, 5, 5),
                (1300, 92, 4, 3), (2423, 1, 1400, 2)]                 # the last: 2800 x 1532 elements, past the grid's 16384 x 256


@pytest.mark.parametrize("Lr,hop,T,B", FRAME_SHAPES)
def test_row_stats_and_frames(Lr, hop, T, B):
    assert (T - 1) * hop + 1024 <= Lr < T * hop + 1024
    yh = _frame_rows(Lr, 0)[:B]
    stats, frames = _crepe_frames(torch.from_numpy(yh).cuda(), hop, T)
    ref = R.row_stats_ref(yh)
    ulps = np.abs(stats.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print(f"\nrow stats Lr {Lr}: |kernel - fp64| in fp32 ulps, (mean, std) per row: {ulps.round(3).tolist()}")
    assert np.all(ulps <= 1.0)
    want = R.frames_fp32(yh, stats, hop, T)
    assert frames.shape == want.shape
    assert np.array_equal(np.isnan(frames), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(frames)[ok], _bits(want)[ok])              # bit-equal: the divide is correctly rounded
    fr = frames.reshape(B, T, 1532)
    assert np.all(_bits(fr[:, :, :254]) == 0) and np.all(_bits(fr[:, :, 1278:]) == 0)    # +0.0, also for the NaN rows
    for b in range(B):
        silent = b >= 3                                                       # the constant and the zero row: 0 / 0
        assert stats[b, 1] == 0 if silent else stats[b, 1] > 0
        assert np.all(np.isnan(fr[b, :, 254:1278])) if silent else np.all(np.isfinite(fr[b, :, 254:1278]))


# ------------------------------------------------------------------------------------------------------------ pitch decode

SPECIAL_BINS = (0, 5, 64, 100, 128, 200, 300, 320, 340, 359)       # the bias is zero there, so that written ties stay ties


def _decode_bias():
    bias = (0.1 * np.random.default_rng(24).standard_normal(360)).astype(np.float32)
    bias[list(SPECIAL_BINS)] = 0.0
    return bias


def _pitch_decode(logits, bias):
    N = logits.shape[0]
    f0_table, cents_table = (t.cuda() for t in ddsp.encoder.pitch_tables())
    z, b = torch.from_numpy(logits).cuda(), torch.from_numpy(bias).cuda()
    probs = torch.full((N, 360), 7.0, device="cuda")
    out = torch.full((3, N), 7.0, device="cuda")
    rc = ddsp._lib.lib().ddsp_pitch_decode(z.data_ptr(), b.data_ptr(), f0_table.data_ptr(), cents_table.data_ptr(), probs.data_ptr(),
                                           out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), N, None)
    ddsp._lib.check(rc, "ddsp_pitch_decode")
    torch.cuda.synchronize()
    return probs.cpu(), out.cpu().numpy()


def _check_decode(logits, bias, expect_bins=None):
    probs, (f0, harm, cents) = _pitch_decode(logits, bias)
    ref = R.decode_ref(logits, bias)
    p = probs.numpy()
    assert np.array_equal(np.isnan(p), np.isnan(ref))
    err = float(np.nanmax(np.abs(p - ref), initial=0.0))
    print(f"\npitch decode N {logits.shape[0]}: worst |p - fp64 sigmoid| {err:.2e}")
    assert err <= 3e-7
    bins = torch.argmax(probs, dim=-1).numpy()                    # of the kernel's own probabilities: first maximum, first NaN
    if expect_bins is not None:
        assert bins.tolist() == list(expect_bins)
    f0_table, cents_table = (t.numpy() for t in ddsp.encoder.pitch_tables())
    rows = np.arange(len(bins))
    assert np.array_equal(_bits(f0), _bits(f0_table[bins])) and np.array_equal(_bits(cents), _bits(cents_table[bins]))
    want = p[rows, bins]
    assert np.array_equal(np.isnan(harm), np.isnan(want)) and np.array_equal(_bits(harm)[~np.isnan(want)], _bits(want)[~np.isnan(want)])
    return bins


@pytest.mark.parametrize("N", [1, 3, 4, 5, 4099])
def test_pitch_decode_random_rows(N):
    logits = (4.0 * np.random.default_rng([N, 25]).standard_normal((N, 360))).astype(np.float32)
    bins = _check_decode(logits, _decode_bias())
    if N == 4099:
        assert len(np.unique(bins)) > 300 and (bins >= 320).any()


def test_pitch_decode_ties_saturation_nan_and_inf():
    rng = np.random.default_rng(26)
    rows, expect = [], []

    def row(expected, **at):
        z = np.clip(rng.standard_normal(360), -3, 3).astype(np.float32)
        for k, v in at.items():
            z[int(k[1:])] = v
        rows.append(z)
        expect.append(expected)

    row(100, b100=9.0, b200=9.0)                                   # two equal maxima in different lanes: the lowest bin
    row(5, b200=9.0, b5=9.0, b100=9.0)                             # three
    row(64, b64=9.0, b128=9.0, b320=9.0)                           # three in one lane (bins 64 apart), the last in the partial pass
    row(100, b300=25.0, b100=30.0, b359=22.0)                      # saturated: the sigmoid is exactly 1.0 in all three
    row(128, b340=np.nan, b128=np.nan)                             # the first NaN wins over any finite value
    row(200, b200=np.nan, b100=50.0)
    row(5, b5=np.inf, b64=-np.inf)                                 # 1 / (1 + 0) and 1 / (1 + inf)
    row(100, b300=np.inf, b100=np.inf)
    row(0, b0=9.0)
    row(359, b359=9.0)
    row(340, b340=9.0)                                             # bins >= 320: only lanes 0 .. 39 make the last pass
    row(0, b0=9.0, b359=9.0)
    rows.append(np.full(360, np.nan, dtype=np.float32))            # all NaN: bin 0
    expect.append(0)
    logits = np.stack(rows)
    probs, _ = _pitch_decode(logits, _decode_bias())
    p = probs.numpy()
    assert p[0, 100] == p[0, 200] and p[3, 100] == p[3, 300] == p[3, 359] == 1.0 and p[6, 5] == 1.0 and p[6, 64] == 0.0
    _check_decode(logits, _decode_bias(), expect)

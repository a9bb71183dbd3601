"""SoftDicePlusBoundarySurface (reference losses.py:66-130, ``--LOSS_MODE region_boundary``): the GPU distance map
(m1_dist_map), the fused loss (m1_dice_bd_fwd / _bwd) and their use by the model and the trainer, against a self-contained fp64
restatement of L:66-130 kept in this file (brute-force Euclidean distances; scipy where it imports)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from util import PKG

L = PKG.hip.lib
LS = PKG.losses
TM = importlib.import_module(PKG.__name__ + ".train_model")
EPS = 1e-7

try:
    from scipy.ndimage import distance_transform_edt as _scipy_edt
except ImportError:                        # pragma: no cover - the brute-force restatement covers the small volumes
    _scipy_edt = None


# ---- fp64 restatement of L:83-130 ---------------------------------------------------------------------------------------------
def edt_brute(mask: np.ndarray) -> np.ndarray:
    """scipy.ndimage.distance_transform_edt(mask) by brute force: for every voxel, the Euclidean distance (unit spacing) to the
    nearest voxel where mask is False (0 there).  Needs at least one False voxel."""
    idx = np.indices(mask.shape).reshape(mask.ndim, -1).T.astype(np.int64)
    bg = idx[~mask.reshape(-1)]
    assert len(bg), "degenerate: no background voxel"
    d2 = ((idx[:, None, :] - bg[None, :, :]) ** 2).sum(-1).min(1)
    return np.sqrt(d2.astype(np.float64)).reshape(mask.shape)


def edt_auto(mask: np.ndarray) -> np.ndarray:
    """Brute force on small volumes (its pairwise table grows with the square of the voxel count), scipy on larger ones."""
    if mask.size <= 4096 or _scipy_edt is None:
        assert mask.size <= 32768, "volume too large for the brute-force restatement"
        return edt_brute(mask)
    return _scipy_edt(mask)


def phi_ref(y: np.ndarray, edt=edt_brute) -> np.ndarray:
    """calc_dist_map_batch(y_true[...,1:]) in fp64: (N,D,H,W,nc) one-hot -> (N,D,H,W,nc-1); 0 for an empty class (L:90) and, the
    package's documented choice, 0 for a class that fills the sample."""
    N, nc = y.shape[0], y.shape[-1]
    out = np.zeros(y.shape[:-1] + (nc - 1,), dtype=np.float64)
    for n in range(N):
        for c in range(1, nc):
            pos = y[n, ..., c].astype(bool)
            if pos.any() and not pos.all():
                neg = ~pos
                out[n, ..., c - 1] = edt(neg) * neg - (edt(pos) - 1) * pos
    return out


def loss_ref(y: torch.Tensor, p: torch.Tensor, phi: torch.Tensor, w, smooth=1e-7) -> torch.Tensor:
    """SoftDicePlusBoundarySurface.loss (L:99-130) in float64 torch: mean over heads of w0 * dice_loss + w1 * boundary loss."""
    nc = y.shape[-1]
    nh = p.shape[-1] // nc
    y = y.double()
    ls = []
    for h in range(nh):
        q = p[..., h * nc:(h + 1) * nc]
        q = q / q.sum(-1, keepdim=True)
        q = torch.clamp(q, EPS, 1 - EPS)
        yf, qf = y[..., 1:].flatten(), q[..., 1:].flatten()
        dice = 1 - 2.0 * (yf * qf).sum() / ((yf + qf).sum() + smooth)
        ls.append(w[0] * dice + w[1] * (q[..., 1:] * phi).sum())
    return torch.stack(ls).mean()


def onehot(lbl: np.ndarray, nc: int) -> np.ndarray:
    return np.stack([(lbl == k) for k in range(nc)], axis=-1).astype(np.float32)


def blobs(shape, nc, seed, n_blobs=3):
    """(N,D,H,W) integer label of random balls of classes 1..nc-1 on background 0."""
    g = np.random.default_rng(seed)
    N, D, H, W = shape
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    lbl = np.zeros(shape, dtype=np.int64)
    for n in range(N):
        for _ in range(n_blobs):
            c = [g.integers(0, s) for s in (D, H, W)]
            r2 = g.integers(1, 10)
            lbl[n][((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2) <= r2] = g.integers(1, nc)
    return lbl


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_class_surface_matches_reference():
    s = LS.SoftDicePlusBoundarySurface()
    assert s.loss_weights == [1.00, 1.50] and s.smooth == pytest.approx(1e-7)
    s2 = LS.SoftDicePlusBoundarySurface(loss_weights=[0.5, 0.5], smooth=1e-5)
    assert s2.loss_weights == [0.5, 0.5] and s2.smooth == 1e-5
    for m in ("calc_dist_map", "calc_dist_map_batch", "dice_loss", "boundary_surface_loss", "DB", "loss"):
        assert callable(getattr(s, m)), m


def test_host_tensors_raise_hip_only():
    s = LS.SoftDicePlusBoundarySurface()
    y = torch.zeros(1, 2, 3, 4, 2); y[..., 0] = 1
    p = torch.full((1, 2, 3, 4, 2), 0.5)
    for call in (lambda: s.loss(y, p), lambda: s.DB(y, p), lambda: s.dice_loss(y, p), lambda: s.boundary_surface_loss(y, p),
                 lambda: s.calc_dist_map_batch(y[..., 1:]), lambda: s.calc_dist_map(y[0, ..., 1:])):
        with pytest.raises(RuntimeError, match="HIP extension only"):
            call()


@pytest.mark.skipif(_scipy_edt is None, reason="scipy not installed")
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_brute_force_edt_equals_scipy(seed):
    """The yardstick itself: the brute-force restatement is scipy's transform."""
    g = np.random.default_rng(seed)
    m = g.random((5, 7, 9)) < 0.8
    m[g.integers(0, 5), g.integers(0, 7), g.integers(0, 9)] = False
    np.testing.assert_array_equal(edt_brute(m), _scipy_edt(m))
    y = onehot(blobs((2, 5, 8, 6), 3, seed), 3)
    np.testing.assert_allclose(phi_ref(y), phi_ref(y, edt=_scipy_edt), rtol=0, atol=1e-12)


def test_abi_rejects_bad_arguments_without_a_gpu():
    lib = L.load()
    bogus = ctypes.c_void_p(256)           # never dereferenced: every call below fails its host-side check before any launch
    assert lib.m1_dist_map_ws_bytes(2, 20, 160, 160, 2) == 2 * 2 * 20 * 160 * 160 * 8
    assert lib.m1_dist_map_ws_bytes(2, 20, 160, 160, 1) == 0
    assert lib.m1_dist_map(None, 0, 1, 2, 3, 4, 2, bogus, bogus, None) == -1
    assert lib.m1_dist_map(bogus, 0, 1, 2, 3, 4, 1, bogus, bogus, None) == -1         # no foreground class
    assert lib.m1_dist_map(bogus, 0, 0, 2, 3, 4, 2, bogus, bogus, None) == -1
    assert lib.m1_dist_map(bogus, 0, 1, 2, 300, 4, 2, bogus, bogus, None) == -2       # line longer than the LDS tiling holds
    assert lib.m1_dist_map(bogus, 0, 1, 257, 3, 4, 2, bogus, bogus, None) == -2
    assert lib.m1_dist_map(bogus, 0, 1, 2, 3, 4, 9, bogus, bogus, None) == -2
    assert lib.m1_dist_map(bogus, 7, 1, 2, 3, 4, 2, bogus, bogus, None) == -2         # dtype
    assert lib.m1_dice_bd_ws_floats(1000, 2) >= 2 * 2 * (2 + 3)
    assert lib.m1_dice_bd_ws_floats(1000, 5) == 0 and lib.m1_dice_bd_ws_floats(0, 1) == 0
    args = (bogus, bogus, 0, bogus, 1000, 1, 2, 0.5, 0.5, 1e-7)
    assert lib.m1_dice_bd_fwd(None, *args[1:], bogus, bogus, None) == -1
    assert lib.m1_dice_bd_fwd(*args[:5], 5, 2, 0.5, 0.5, 1e-7, bogus, bogus, None) == -2          # too many heads
    assert lib.m1_dice_bd_fwd(*args[:6], 1, 0.5, 0.5, 1e-7, bogus, bogus, None) == -1              # nc < 2
    assert lib.m1_dice_bd_fwd(*args, ctypes.c_void_p(260), bogus, None) == -1                     # ws not 8-byte aligned
    assert lib.m1_dice_bd_fwd(*args, None, bogus, None) == -1
    assert lib.m1_dice_bd_bwd(*args, bogus, None, bogus, None) == -1
    assert lib.m1_dice_bd_bwd(*args[:2], 3, *args[3:], bogus, bogus, bogus, None) == -2           # dtype


# ---- GPU: distance map ----------------------------------------------------------------------------------------------------------
def _check_phi(got: torch.Tensor, ref: np.ndarray):
    g = got.cpu().numpy().astype(np.float64)
    assert g.shape == ref.shape
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    bad = np.abs(g - ref) > ulp
    assert not bad.any(), (int(bad.sum()), float(np.abs(g - ref).max()))
    out = ref > 0                          # outside: the squared distance underneath is an integer, and exact
    np.testing.assert_array_equal(np.rint(g[out] ** 2), np.rint(ref[out] ** 2))
    ins = ref <= 0
    np.testing.assert_array_equal(np.rint((1 - g[ins]) ** 2), np.rint((1 - ref[ins]) ** 2))


def _cases():
    c = {}
    for s in (0, 1, 2):
        c[f"blobs{s}"] = onehot(blobs((2, 6, 11, 13), 2, s), 2)
    lbl = np.zeros((1, 5, 9, 10), np.int64)
    lbl[0, 0, 2:5, 3:6] = 1; lbl[0, 4, 4:8, 2:9] = 1; lbl[0, 1:4, 0, 4] = 1; lbl[0, 2, 3, 9] = 1; lbl[0, 1:3, 8, 0:3] = 1
    lbl[0, 2, 5, 0] = 1
    c["every_face"] = onehot(lbl, 2)
    lbl = np.zeros((1, 7, 12, 12), np.int64); lbl[0, 1:3, 1:4, 1:3] = 1; lbl[0, 5:7, 8:12, 9:11] = 1; lbl[0, 3, 6, 6] = 1
    c["components"] = onehot(lbl, 2)
    lbl = np.zeros((2, 6, 7, 8), np.int64); lbl[0, 3, 2, 5] = 1; lbl[1, 0, 6, 0] = 1
    c["single_voxel"] = onehot(lbl, 2)
    lbl = np.zeros((2, 4, 6, 5), np.int64); lbl[1, 1:3, 2:4, 1:4] = 1          # sample 0 empty: phi == 0
    c["empty_class"] = onehot(lbl, 2)
    y = np.zeros((2, 3, 5, 4, 2), np.float32); y[0, ..., 1] = 1; y[1, ..., 0] = 1; y[1, 1, 2, 2] = [0, 1]
    c["all_foreground"] = y                                                 # sample 0: the class fills it -> phi == 0
    c["nc3"] = onehot(blobs((2, 5, 9, 10), 3, 7), 3)
    c["soft_labels"] = onehot(blobs((1, 4, 8, 8), 2, 3), 2) * 0.3         # astype(bool): soft labels count as foreground
    c["d1"] = onehot(blobs((2, 1, 12, 15), 2, 4, n_blobs=2), 2)
    c["w1"] = onehot(blobs((1, 9, 10, 1), 2, 5, n_blobs=2), 2)
    c["h1"] = onehot(blobs((1, 6, 1, 17), 2, 6, n_blobs=2), 2)
    c["long_w"] = onehot(blobs((1, 2, 3, 200), 2, 8, n_blobs=2), 2)
    return c


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dist_map_exact(dev, name, dtype):
    y = CASES[name]
    ref = phi_ref(y)
    got = PKG.hip.ops.dist_map(torch.from_numpy(y).to(dtype).to(dev))
    _check_phi(got, ref)
    if name == "empty_class":
        assert float(got[0].abs().max()) == 0.0
    if name == "all_foreground":
        assert float(got[0].abs().max()) == 0.0 and float(got[1].abs().max()) > 0


@pytest.mark.gpu
def test_calc_dist_map_methods(dev):
    s = LS.SoftDicePlusBoundarySurface()
    y = CASES["nc3"]
    ref = phi_ref(y)
    yt = torch.from_numpy(y).to(dev)
    _check_phi(s.calc_dist_map_batch(yt[..., 1:]), ref)
    _check_phi(s.calc_dist_map(yt[1, ..., 1:]), ref[1])


@pytest.mark.gpu
@pytest.mark.skipif(_scipy_edt is None, reason="scipy not installed")
def test_dist_map_bench_shape_against_scipy(dev):
    """The full bench shape (2,20,160,160,2): the training data's ball lesions plus random blobs, against scipy."""
    lbl = blobs((2, 20, 160, 160), 2, 11, n_blobs=6)
    g = np.random.default_rng(12)
    zz, yy, xx = np.meshgrid(np.arange(20), np.arange(160), np.arange(160), indexing="ij")
    lbl[1][((zz - 10) ** 2 + (yy - g.integers(20, 140)) ** 2 + (xx - g.integers(20, 140)) ** 2) <= 36] = 1
    y = onehot(lbl, 2)
    got = PKG.hip.ops.dist_map(torch.from_numpy(y).to(dev))
    _check_phi(got, phi_ref(y, edt=_scipy_edt))


# ---- GPU: loss and gradient -----------------------------------------------------------------------------------------------------
def _problem(shape, nc, nheads, seed, clip=True):
    g = np.random.default_rng(seed)
    y = onehot(blobs(shape, nc, seed, n_blobs=4), nc)
    logits = g.standard_normal(shape + (nheads * nc,)) * 2.0
    p = np.exp(logits.reshape(shape + (nheads, nc)))
    p = p / p.sum(-1, keepdims=True)
    if clip:                                # a few voxels per head driven into the clip range at each end
        flat = p.reshape(-1, nheads, nc)
        for h in range(nheads):
            ix = g.choice(flat.shape[0], 8, replace=False)
            flat[ix[:4], h, 1] = 1e-10
            flat[ix[4:], h, :] = 1e-10
            flat[ix[4:], h, 1] = 1.0
    return y, p.reshape(shape + (nheads * nc,)).astype(np.float32)


def _check_loss(dev, y, p, w, ydtype=torch.float32):
    phi = torch.from_numpy(phi_ref(y, edt=edt_auto))
    pd = torch.from_numpy(p).double().requires_grad_(True)
    lr = loss_ref(torch.from_numpy(y), pd, phi, w)
    lr.backward()
    pg = torch.from_numpy(p).to(dev).requires_grad_(True)
    l = LS.SoftDicePlusBoundarySurface(loss_weights=w).loss(torch.from_numpy(y).to(ydtype).to(dev), pg)
    l.backward()
    l, lr = float(l.detach()), float(lr.detach())
    assert abs(l - lr) <= 1e-5 * abs(lr), (l, lr)
    ge, gr = pg.grad.double().cpu(), pd.grad
    assert float((ge - gr).abs().max()) <= 1e-5 * float(gr.abs().max()), (float((ge - gr).abs().max()), float(gr.abs().max()))
    return l, pg.grad


@pytest.mark.gpu
@pytest.mark.parametrize("nheads", [1, 2, 4])
@pytest.mark.parametrize("nc", [2, 3])
def test_loss_and_gradient(dev, nheads, nc):
    y, p = _problem((2, 5, 12, 14), nc, nheads, 100 + 10 * nheads + nc)
    _check_loss(dev, y, p, [0.5, 0.5])
    if nheads == 2:
        _check_loss(dev, y, p, [1.0, 1.5], ydtype=torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.skipif(_scipy_edt is None, reason="scipy not installed")
def test_loss_full_size(dev):
    y, p = _problem((2, 20, 160, 160), 2, 1, 7)
    _check_loss(dev, y, p, [0.5, 0.5])


@pytest.mark.gpu
def test_single_head_methods(dev):
    """dice_loss, boundary_surface_loss and DB of ONE head (L:99-119) against the restatement's two terms."""
    y, p = _problem((1, 4, 10, 9), 2, 2, 5, clip=False)
    s = LS.SoftDicePlusBoundarySurface(loss_weights=[0.7, 0.2])
    yt, pt = torch.from_numpy(y).to(dev), torch.from_numpy(p).to(dev)
    phi = torch.from_numpy(phi_ref(y))
    p0 = torch.from_numpy(p[..., :2]).double()
    dice = float(loss_ref(torch.from_numpy(y), p0, phi, [1.0, 0.0]))
    bd = float(loss_ref(torch.from_numpy(y), p0, phi, [0.0, 1.0]))
    assert float(s.dice_loss(yt, pt)) == pytest.approx(dice, rel=1e-5)
    assert float(s.boundary_surface_loss(yt, pt)) == pytest.approx(bd, rel=1e-5)
    assert float(s.DB(yt, pt)) == pytest.approx(0.7 * dice + 0.2 * bd, rel=1e-5)


@pytest.mark.gpu
def test_deterministic(dev):
    y, p = _problem((2, 8, 40, 40), 2, 4, 3)
    s = LS.SoftDicePlusBoundarySurface(loss_weights=[0.5, 0.5])
    out = []
    for _ in range(2):
        pg = torch.from_numpy(p).to(dev).requires_grad_(True)
        l = s.loss(torch.from_numpy(y).to(dev), pg)
        l.backward()
        out.append((l.detach().clone(), pg.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_graph_capture_replays_bit_exact(dev):
    """Forward + backward of the loss captured with torch.cuda.graph; new labels copied into the static buffer before each of three
    replays; every replay equals the eager result bit for bit, and the graph holds no memset node."""
    s = LS.SoftDicePlusBoundarySurface(loss_weights=[0.5, 0.5])
    shape = (2, 6, 32, 32)
    probs = [_problem(shape, 2, 2, 40 + i) for i in range(4)]
    y_s = torch.from_numpy(probs[0][0]).to(dev)
    p_s = torch.from_numpy(probs[0][1]).to(dev).requires_grad_(True)

    def step():
        p_s.grad = None
        l = s.loss(y_s, p_s)
        l.backward()
        return l
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr):
        l_s = step()
    g_s = p_s.grad
    hist = PKG.hip.graphs.assert_no_memset_nodes(gr)
    assert hist.get("kernel", 0) >= 5, hist                 # 3 distance-map passes, forward + finish, backward
    gr.instantiate()
    for i in range(1, 4):
        y_new, p_new = probs[i]
        y_s.copy_(torch.from_numpy(y_new).to(dev)); p_s.data.copy_(torch.from_numpy(p_new).to(dev))
        gr.replay()
        torch.cuda.synchronize()
        pe = torch.from_numpy(p_new).to(dev).requires_grad_(True)
        le = s.loss(torch.from_numpy(y_new).to(dev), pe)
        le.backward()
        assert torch.equal(l_s, le.detach()) and torch.equal(g_s, pe.grad), i
    del gr


# ---- GPU: whole model and trainer -----------------------------------------------------------------------------------------------
def _train(dev, prob, deep_supervision, steps=20):
    T = TM
    rng = np.random.default_rng(0)
    dims = (8, 32, 32)
    cases = [T.synthetic_case(rng, dims, 3, 2) for _ in range(2)]
    gen = T.batches(T.custom_data_generator(cases, probabilistic=prob, mode='train'), 2, dev)
    PKG.unets.network_blocks.set_init_seed(0)
    m = PKG.unets.networks.M1(input_spatial_dims=dims, input_channels=3 + (1 if prob else 0), num_classes=2, dropout_rate=0.0,
                              filters=(8, 16, 32, 64, 128), strides=((1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2), (2, 2, 2)),
                              dense_skip=True, deep_supervision=deep_supervision, probabilistic=prob,
                              prob_latent_dims=(3, 2, 1, 0), summary=False).to(dev)
    m.set_compute_dtype(torch.float32)
    seen = []
    dbl = LS.SoftDicePlusBoundarySurface(loss_weights=[0.5, 0.5]).loss

    def spy(yt, yp):
        seen.append(int(yp.shape[-1]) // int(yt.shape[-1]))
        return dbl(yt, yp)
    losses = [spy] + ([LS.EvidenceLowerBound().loss] if prob else [])
    m.compile(optimizer=PKG.optim.Adam(learning_rate=1e-3, amsgrad=True), loss=losses, loss_weights=[1.0, 10.0][:len(losses)])
    x, y = next(gen)
    hist = [m.train_step(x, y)["loss"] for _ in range(steps)]
    return hist, seen


@pytest.mark.gpu
@pytest.mark.parametrize("prob,ds", [(True, False), (False, True)])
def test_train_step_reduces_loss(dev, prob, ds):
    hist, seen = _train(dev, prob, ds)
    assert np.isfinite(hist).all()
    assert hist[-1] < hist[0], hist
    assert seen and (seen[0] == 1 if prob else seen[0] > 1), seen      # deep supervision: several heads reach the loss


@pytest.mark.gpu
def test_trainer_region_boundary(dev, tmp_path):
    T = TM
    wd = str(tmp_path) + "/"
    argv = ["--WEIGHTS_DIR", wd, "--NAME", "rb", "--FOLDS", "0", "--UNET_FEATURE_CHANNELS", "8", "16", "32", "64", "128",
            "--UNET_PROBABILISTIC", "1", "--UNET_DENSE_SKIP", "1", "--SYNTHETIC_SAMPLES", "4", "--IMAGE_SPATIAL_DIMS", "4", "32", "32",
            "--BATCH_SIZE", "2", "--UNET_DROPOUT_RATE", "0", "--WEIGHTS_MIN_EPOCH", "1", "--STORE_WEIGHTS_PER_N_EPOCHS", "1",
            "--COMPUTE_DTYPE", "fp32", "--NUM_EPOCHS", "2", "--LOSS_MODE", "region_boundary", "--DSC_BD_LOSS_WEIGHTS", "0.5", "0.5",
            "--FOCAL_LOSS_ALPHA", "1.0"]                       # the alpha length check belongs to distribution_focal only
    (model, hist, _), = T.main(argv)
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(hist.history["loss"]))
    assert any(f.startswith("model_weights_") and f.endswith(".npz") for f in os.listdir(os.path.join(wd + "rb", "F1")))


def test_trainer_rejects_unknown_loss_mode(tmp_path):
    T = TM
    a = T.build_parser().parse_args(["--WEIGHTS_DIR", str(tmp_path) + "/", "--NAME", "x", "--LOSS_MODE", "dice",
                                     "--SYNTHETIC_SAMPLES", "2", "--IMAGE_SPATIAL_DIMS", "4", "32", "32"])
    with pytest.raises(NotImplementedError, match="region_boundary"):
        T.train_fold(a, 0, torch.device("cpu"))

"""Host mirror of the reference's GNN dataset (`dataset/dataset_gnn_dyn.py:27-201`, row x4), the training data of
train_gnn_dyn.py.  Same name and arguments, so a script swaps one import:

    from dyn_res_pile_manip_amd.dataset_gnn_dyn import ParticleDataset

  ParticleDataset(data_dir, config, phase, cam)   :27-63  phases, `__len__`, the idx -> (episode, timestep) mapping
  ParticleDataset.read_particles(path)            :65-78  a particle file in the camera frame (host numpy)
  ParticleDataset[idx]                            :80-201 the 6-tuple (states, states_delta, attrs, particle_num,
                                                          particle_den, color_imgs), numpy
  ParticleDataset.get_batch(indices)              collate_fn([ds[i] for i in indices]) in ONE device call
  DeviceLoader(dataset, batch_size, shuffle)      the DataLoader of train/train_gnn_dyn.py:94-100
  DepthDataset(data_dir, config, phase, cam)      untracked samples from the depth PNGs and actions.p alone (no counterpart)

What the reference computes per sample -- depth2fgpcd, fps_rad (a Python loop over the whole cloud), recenter (a dense
float64 distance matrix), the KDTree query, the gather and the push formula -- runs in `drp_ptcl_dataset_batch` on the
MI355X for many samples at once (include/drp.h).  The host decodes the files (PNG, .npy, actions.p: a thread pool of at
most 16 threads), counts the foreground (the sampler's start is drawn from it) and forms the push frames in float64 with
opengl2cam's own expression.  No cv2, dgl, scipy or FleX is needed.

Random draws are the reference's calls in its order on numpy's global generator: per sample np.random.uniform(15, 6500),
then np.random.randint(n_fg).  Under the same seed the same samples come out.  One deliberate difference: DeviceLoader
draws from ONE numpy stream in sample order, as DataLoader(num_workers=0) does; the reference's forked workers each draw
from a copy of the parent's global numpy state.

DepthDataset is the data path of a recorded robot episode, which holds depth images and pushes and no simulator particles: every
frame of a window goes through depth2fgpcd -> fps_rad -> recenter (`drp_ptcl_dataset_frames`), frame 0 is the state, frames
1..T-1 are the Chamfer targets.  Its draws per sample: np.random.uniform(15, 6500), then np.random.randint(n_fg_t) for the frames
t = 0..T-1 in order, so under one seed the first sample's frame-0 cloud is the one ParticleDataset samples.
"""
import os
import pickle

import numpy as np

from .engine import default_engine
from .train_gnn_dyn import PaddedBatch, collate_fn

PARTICLE_DEN_MIN = 15        # :89
PARTICLE_DEN_MAX = 6500      # :90
PUSHER_W = 0.8 / 24.0        # :138
MAX_THREADS = 16

_OPENCV_T_OPENGL = np.array([[1, 0, 0, 0],
                             [0, -1, 0, 0],
                             [0, 0, -1, 0],
                             [0, 0, 0, 1]])


def cam_T(cam_extrinsic):
    """inv(opencv_T_world) as read_particles (:69-76) and opengl2cam (utils.py:479-489) form it"""
    opencv_T_world = np.matmul(np.linalg.inv(cam_extrinsic), _OPENCV_T_OPENGL)
    return np.linalg.inv(opencv_T_world)


def opengl2cam(pcd, cam_extrinsic, global_scale):
    """utils.py:479-489"""
    return np.matmul(cam_T(cam_extrinsic), np.concatenate([pcd, np.ones((pcd.shape[0], 1))], axis=1).T).T[:, :3] \
        / global_scale


def push_frame(action, cam_extrinsic, global_scale):
    """:134-147 for one push (sx, sy, ex, ey) -> [10] float64: s_3d_cam, e_3d_cam, push_dir_cam (unit), push_l.  A zero-length
    push gives NaN directions (the device refuses it, where the reference exits)."""
    s, e, h = action[:2], action[2:], 0.0
    s_3d = np.array([s[0], h, -s[1]])
    e_3d = np.array([e[0], h, -e[1]])
    s_3d_cam = opengl2cam(s_3d[None, :], cam_extrinsic, global_scale)[0]
    e_3d_cam = opengl2cam(e_3d[None, :], cam_extrinsic, global_scale)[0]
    push_dir_cam = e_3d_cam - s_3d_cam
    push_l = np.linalg.norm(push_dir_cam)
    with np.errstate(divide='ignore', invalid='ignore'):
        push_dir_cam = push_dir_cam / np.linalg.norm(push_dir_cam)
    return np.concatenate([s_3d_cam, e_3d_cam, push_dir_cam, [push_l]])


def count_fg(depth_u16, global_scale):
    """foreground pixels of a depth PNG by the float64 rule of :97-98 and utils.py:496"""
    d = depth_u16 / (global_scale * 1000.0)
    return int(np.count_nonzero((d < 0.599 / 0.8) & (d > 0)))


def read_depth(path):
    """cv2.imread(path, cv2.IMREAD_ANYDEPTH) of a 16-bit PNG -> uint16 [h, w]"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim != 2:
        raise ValueError('%s: a depth PNG has one channel, found shape %s' % (path, a.shape))
    if a.dtype != np.uint16:
        if a.min() < 0 or a.max() > 65535:
            raise ValueError('%s: depth values outside uint16' % path)
        a = a.astype(np.uint16)
    return np.ascontiguousarray(a)


def read_color(path):
    """cv2.imread(path) -> uint8 [h, w, 3] BGR"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert('RGB'))
    return np.ascontiguousarray(a[..., ::-1])


class ParticleDataset(object):
    """dataset/dataset_gnn_dyn.py:27-201 with the per-sample work on the device.  `cam` = (cam_params [fx, fy, cx, cy],
    cam_extrinsic 4x4) as FlexEnv gives them; engine: the context to run on (default: the process's one)."""

    default_chunk = 64           # samples per device call of a DeviceLoader

    def __init__(self, data_dir, config, phase, cam, engine=None, load_color=False):
        self.config = config
        n_episode = config['dataset']['n_episode']
        n_timestep = config['dataset']['n_timestep']
        self.global_scale = config['dataset']['global_scale']
        train_valid_ratio = config['train']['train_valid_ratio']
        n_train = int(n_episode * train_valid_ratio)
        n_valid = n_episode - n_train
        if phase == 'train':
            self.epi_st_idx = 0
            self.n_episode = n_train
        elif phase == 'valid':
            self.epi_st_idx = n_train
            self.n_episode = n_valid
        else:
            raise AssertionError("Unknown phase %s" % phase)
        self.n_timestep = n_timestep + 1
        self.n_his = config['train']['n_history']
        self.n_roll = config['train']['n_rollout']
        self.data_dir = data_dir
        self.screenHeight = 720
        self.screenWidth = 720
        self.img_channel = 1
        self.cam_params, self.cam_extrinsic = cam
        self.load_color = bool(load_color)
        self._engine = engine
        self._T_cam = cam_T(np.asarray(self.cam_extrinsic))

    @property
    def engine(self):
        return self._engine if self._engine is not None else default_engine()

    def __len__(self):
        return self.n_episode * (self.n_timestep - self.n_his - self.n_roll + 1)

    def locate(self, idx):
        """:93-95 -> (episode, first timestep)"""
        if not 0 <= idx < len(self):
            raise IndexError('index %d outside a dataset of %d samples' % (idx, len(self)))
        offset = self.n_timestep - self.n_his - self.n_roll + 1
        return idx // offset + self.epi_st_idx, idx % offset

    def read_particles(self, particles_path):
        """:65-78 on the host -> [n, 3] float64 in the camera frame"""
        particles = np.load(particles_path).reshape(-1, 4)
        particles[:, 3] = 1.0
        return np.matmul(self._T_cam, particles.T).T[:, :3] / self.global_scale

    def _path(self, ep, name):
        return os.path.join(self.data_dir, '%d' % ep, name)

    def load(self, idx):
        """The files of sample idx, decoded (thread-safe, no random draw): depth uint16, its foreground count, the T
        particle frames [T, n, 4] float32, the T-1 push frames [T-1, 10], the raw pushes [T-1, 4] (sx, sy, ex, ey as pickled),
        colour images (load_color) or None."""
        ep, t0 = self.locate(idx)
        T = self.n_his + self.n_roll
        with open(self._path(ep, 'actions.p'), 'rb') as fp:
            actions = pickle.load(fp)
        depth = read_depth(self._path(ep, '%d_depth.png' % t0))
        frames = [np.load(self._path(ep, '%d_particles.npy' % i)).reshape(-1, 4) for i in range(t0, t0 + T)]
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError('episode %d: the particle count changes between frames %d..%d' % (ep, t0, t0 + T - 1))
        push = np.stack([push_frame(np.asarray(actions[i], dtype=np.float64), self.cam_extrinsic, self.global_scale)
                         for i in range(t0, t0 + T - 1)])
        color = None
        if self.load_color:
            color = np.zeros((T, 720, 720, 3), np.uint8)
            for i in range(t0, t0 + T):
                color[i - t0] = read_color(self._path(ep, '%d_color.png' % i))
        return {'episode': ep, 'depth': depth, 'n_fg': count_fg(depth, self.global_scale),
                'particles': np.stack(frames).astype(np.float32, copy=False), 'push': push,
                'actions': np.asarray([actions[i] for i in range(t0, t0 + T - 1)], dtype=np.float64).reshape(T - 1, 4),
                'color': color}

    @staticmethod
    def draw(sample):
        """the reference's draws for one loaded sample, in its order: particle_den (:91), then fps_rad's start
        (utils.py:442).  An empty foreground draws no start (the reference's randint(0) raises; the device refuses it)."""
        den = np.random.uniform(PARTICLE_DEN_MIN, PARTICLE_DEN_MAX)
        init = np.random.randint(sample['n_fg']) if sample['n_fg'] > 0 else 0
        return den, init

    def run(self, samples, draws):
        """one device call for loaded samples and their draws -> (states [B,T,n_max,3], states_delta, counts)"""
        return self.engine.ptcl_dataset_batch(
            np.stack([s['depth'] for s in samples]), self.global_scale, self.cam_params, self._T_cam,
            [s['particles'] for s in samples], [1 / np.sqrt(d[0]) for d in draws], [d[1] for d in draws],
            [s['n_fg'] for s in samples], np.stack([s['push'] for s in samples]),
            episode=[s['episode'] for s in samples])

    def tuples(self, samples, draws):
        """one device call -> the per-sample tuples of __getitem__ (views of the call's outputs), in order"""
        states, sdelta, counts = self.run(samples, draws)
        T = states.shape[1]
        return [(states[j, :, :int(counts[j])], sdelta[j, :, :int(counts[j])], np.zeros((T, int(counts[j])), np.float32),
                 int(counts[j]), draws[j][0], s['color']) for j, s in enumerate(samples)]

    @staticmethod
    def collate(data, actions):
        """per-sample tuples and their raw pushes [T-1, 4] -> the batch a loader yields (collate_fn's tuple is the reference's:
        the pushes are attached)"""
        out = collate_fn(data)
        out.actions = np.stack(actions).astype(np.float32)
        return out

    def __getitem__(self, idx):
        sample = self.load(idx)
        den, init = self.draw(sample)
        states, sdelta, counts = self.run([sample], [(den, init)])
        n = int(counts[0])
        T = self.n_his + self.n_roll
        return (states[0, :, :n].copy(), sdelta[0, :, :n].copy(), np.zeros((T, n), np.float32), n, den,
                sample['color'])

    def check_limit(self, n):
        """refuses more samples than one device call takes"""
        if n > 1024:
            raise ValueError('get_batch takes at most 1024 samples per call, got %d' % n)

    def load_and_draw(self, indices, pool=None):
        """the samples of a get_batch, decoded (through `pool` if given), and their draws in sample order"""
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError('get_batch needs at least one index')
        self.check_limit(len(indices))
        samples = list(pool.map(self.load, indices)) if pool is not None else [self.load(i) for i in indices]
        return samples, [self.draw(s) for s in samples]

    def get_batch(self, indices, pool=None):
        """collate_fn([self[i] for i in indices]) (train/train_gnn_dyn.py:20-45) from the same numpy state, in one
        device call; `pool`: an executor for the decoding."""
        samples, draws = self.load_and_draw(indices, pool)
        states, sdelta, counts = self.run(samples, draws)
        B, T, n_max, _ = states.shape
        imgs = None if samples[0]['color'] is None else np.stack([s['color'] for s in samples]).astype(np.float32)
        batch = PaddedBatch((states, sdelta, np.zeros((B, T, n_max), np.float32), counts.astype(np.int32),
                             np.asarray([d[0] for d in draws], dtype=np.float32), imgs))
        batch.offsets = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        batch.actions = np.stack([s['actions'] for s in samples]).astype(np.float32)
        return batch


class DepthDataset(ParticleDataset):
    """Untracked training samples straight from recorded depth frames: the phases, `__len__` and `locate` of ParticleDataset, but
    a sample is read from the T = n_his + n_rollout depth PNGs of its window and actions.p alone -- no `*_particles.npy`, no
    colour image.  Every frame becomes a cloud by the reference's own chain depth2fgpcd -> fps_rad -> recenter
    (dataset/dataset_gnn_dyn.py:97-101) on the device (Engine.ptcl_dataset_frames): frame 0 at radius 1/sqrt(den), the frames
    after it, the Chamfer targets, at 1/sqrt(den * target_den_scale).  Batches are collate_untracked's and carry
    `depth_only = True`: there are no recorded impulses, so they train with loss='chamfer', impulses='actions' only."""

    default_chunk = 16           # 16 samples x 6 frames at 720 x 720 upload 100 MB and hold 0.4 GB of clouds on the device

    def __init__(self, data_dir, config, phase, cam, engine=None, target_den_scale=1.0):
        ParticleDataset.__init__(self, data_dir, config, phase, cam, engine=engine)
        if not (float(target_den_scale) > 0.0 and np.isfinite(target_den_scale)):
            raise ValueError('target_den_scale must be positive and finite, got %r' % (target_den_scale,))
        self.target_den_scale = float(target_den_scale)

    def load(self, idx):
        """The files of sample idx, decoded (thread-safe, no random draw): the T depth frames uint16 [T, h, w], their
        foreground counts [T], the raw pushes [T-1, 4]."""
        ep, t0 = self.locate(idx)
        T = self.n_his + self.n_roll
        with open(self._path(ep, 'actions.p'), 'rb') as fp:
            actions = pickle.load(fp)
        depth = np.stack([read_depth(self._path(ep, '%d_depth.png' % i)) for i in range(t0, t0 + T)])
        return {'episode': ep, 'depth': depth, 'n_fg': [count_fg(d, self.global_scale) for d in depth],
                'actions': np.asarray([actions[i] for i in range(t0, t0 + T - 1)], dtype=np.float64).reshape(T - 1, 4),
                'color': None}

    def check_limit(self, n):
        T = self.n_his + self.n_roll
        if n * T > 1024:
            raise ValueError('get_batch takes at most 1024 frames per call, got %d samples of %d' % (n, T))

    @staticmethod
    def draw(sample):
        """the draws of one loaded sample: particle_den as ParticleDataset.draw, then every frame's sampler start in frame
        order -> (den, [init_0 .. init_T-1]).  A frame without foreground draws no start (the device refuses it)."""
        den = np.random.uniform(PARTICLE_DEN_MIN, PARTICLE_DEN_MAX)
        return den, [np.random.randint(n) if n > 0 else 0 for n in sample['n_fg']]

    def radii(self, den, T):
        """fps_rad's radius of every frame of a sample: [T] float64"""
        r = np.full((T,), 1 / np.sqrt(den * self.target_den_scale), np.float64)
        r[0] = 1 / np.sqrt(den)
        return r

    def run(self, samples, draws):
        """one device call for loaded samples and their draws -> (clouds [B,T,n_max,3], counts [B,T])"""
        depth = np.stack([s['depth'] for s in samples])
        return self.engine.ptcl_dataset_frames(
            depth, self.global_scale, self.cam_params, np.stack([self.radii(d[0], depth.shape[1]) for d in draws]),
            [d[1] for d in draws], [s['n_fg'] for s in samples], episode=[s['episode'] for s in samples])

    def tuples(self, samples, draws):
        """one device call -> the per-sample tuples of __getitem__ (copies), in order"""
        clouds, counts = self.run(samples, draws)
        T = clouds.shape[1]
        out = []
        for j in range(len(samples)):
            n = int(counts[j, 0])
            states = np.zeros((T, n, 3), np.float32)
            states[0] = clouds[j, 0, :n]
            out.append((states, np.zeros((T - 1, n, 3), np.float32), np.zeros((T, n), np.float32), n, draws[j][0], None,
                        [clouds[j, t, :int(counts[j, t])].copy() for t in range(1, T)]))
        return out

    @staticmethod
    def collate(data, actions):
        from .train_gnn_dyn import collate_untracked
        out = collate_untracked(data, actions=np.stack(actions))
        out.depth_only = True
        return out

    def __getitem__(self, idx):
        """-> (states [T, n, 3] with step 0 filled, states_delta zeros, attrs zeros, n, particle_den, None, targets: the T-1
        clouds [m_t, 3] of the frames after the first): what collate_untracked takes"""
        sample = self.load(idx)
        return self.tuples([sample], [self.draw(sample)])[0]

    def get_batch(self, indices, pool=None):
        """collate_untracked([self[i] for i in indices]) from the same numpy state, in one device call, with the raw pushes as
        `.actions` and `depth_only = True`; `pool`: an executor for the decoding."""
        samples, draws = self.load_and_draw(indices, pool)
        return self.collate(self.tuples(samples, draws), [s['actions'] for s in samples])


def drop_correspondence(sample, rng, keep=(0.6, 1.0)):
    """A tracked sample (the 6-tuple of ParticleDataset[idx]) -> an untracked one: the same six fields, then `targets`, a list of
    n_rollout clouds.  Target t is a random subset of the rows of states[t + 1] in random order; its size is drawn uniformly
    from keep x n (at least one row).  What a pile re-sampled after every push, or a depth camera, gives: points of the next
    state without the particle they belong to (train_gnn_dyn.collate_untracked, train(loss='chamfer')).  rng: a
    numpy.random.Generator."""
    states = np.asarray(sample[0])
    n = int(sample[3])
    targets = []
    for t in range(1, states.shape[0]):
        m = int(np.clip(int(round(rng.uniform(keep[0], keep[1]) * n)), 1, n))
        targets.append(np.ascontiguousarray(states[t, :n][rng.permutation(n)[:m]], dtype=np.float32))
    return tuple(sample[:6]) + (targets,)


def track_clouds(engine, clouds, counts):
    """The bridge from untracked clouds back to the tracked tools: clouds [T, N, 3] (the frames of one untracked window, padded)
    with counts [T] real rows each -> perms [T, n] int64 with clouds[t, perms[t, i]] the row of frame t that is particle i of
    frame 0 (perms[0] = arange(n)).  Consecutive frames are paired by Engine.cloud_match, the one-to-one matching at the least
    total squared distance, all T - 1 pairs in one call, and the partners are chained; clouds[t, perms[t]] is then a tracked
    window that loss='mse' and train_grad_f64 can read.  A window whose counts are not all equal has rows without a partner and
    is refused (ValueError)."""
    clouds = np.ascontiguousarray(clouds, dtype=np.float32)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if clouds.ndim != 3 or clouds.shape[2] != 3 or counts.shape[0] != clouds.shape[0]:
        raise ValueError('clouds must be [T, N, 3] with one count per frame, got %s and %d counts' % (clouds.shape, counts.shape[0]))
    if clouds.shape[0] < 1 or (counts != counts[0]).any():
        raise ValueError('a window is tracked only where all its counts are equal, got %s' % (counts.tolist(),))
    n = int(counts[0])
    perms = np.empty((clouds.shape[0], n), np.int64)
    perms[0] = np.arange(n)
    if clouds.shape[0] > 1:
        out = engine.cloud_match(clouds[:-1], clouds[1:], counts[:-1], counts[1:], want_match=True)
        for t in range(1, clouds.shape[0]):
            perms[t] = out['match_pq'][t - 1][perms[t - 1]]
    return perms


class UntrackedLoader(object):
    """A loader of collated tracked batches (DeviceLoader) -> untracked ones: every sample of every batch goes through
    drop_correspondence (one numpy Generator, in sample order), the batch through collate_untracked.  reseed: every pass starts
    from the seed again (a validation set that stays the same from epoch to epoch)."""

    def __init__(self, loader, seed=0, keep=(0.6, 1.0), reseed=False):
        self.loader = loader
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.keep = keep
        self.reseed = bool(reseed)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from .train_gnn_dyn import collate_untracked
        if self.reseed:
            self.rng = np.random.default_rng(self.seed)
        for batch in self.loader:
            states, sdelta, attrs, nums, dens, imgs = [batch[i] for i in range(6)]
            data = []
            for b, n in enumerate(np.asarray(nums)):
                n = int(n)
                data.append(drop_correspondence((states[b][:, :n], sdelta[b][:, :n], attrs[b][:, :n], n, dens[b],
                                                 None if imgs is None else imgs[b]), self.rng, self.keep))
            yield collate_untracked(data, actions=getattr(batch, 'actions', None))


class _Indices(object):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class DeviceLoader(object):
    """DataLoader(dataset, batch_size, shuffle, collate_fn=collate_fn) (train/train_gnn_dyn.py:94-100) on the device.
    The sample order is torch's: a DataLoader over the indices (RandomSampler / SequentialSampler) consumes torch's
    generator exactly as the reference's does.  `chunk` samples go to the device per call (fps_rad runs one workgroup per
    sample: a chunk fills the CUs) and come back as batches of batch_size; the chunk size does not change the output.
    Decoding runs on `threads` (at most 16) threads, one chunk ahead of the device.  chunk None: the dataset's default_chunk
    (ParticleDataset 64; DepthDataset, whose samples are T images each, 16).  A DepthDataset's batches are collate_untracked's."""

    def __init__(self, dataset, batch_size, shuffle=False, chunk=None, threads=8, drop_last=False):
        if int(batch_size) < 1:
            raise ValueError('batch_size must be >= 1, got %r' % (batch_size,))
        if chunk is None:
            chunk = dataset.default_chunk
        if int(chunk) < 1 or int(chunk) > 1024:
            raise ValueError('chunk must be in 1..1024, got %r' % (chunk,))
        if int(threads) < 1 or int(threads) > MAX_THREADS:
            raise ValueError('threads must be in 1..%d, got %r' % (MAX_THREADS, threads))
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.chunk = int(chunk)
        self.threads = int(threads)
        self.drop_last = bool(drop_last)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def index_batches(self):
        import torch.utils.data as tud
        return list(tud.DataLoader(_Indices(len(self.dataset)), batch_size=self.batch_size, shuffle=self.shuffle,
                                   drop_last=self.drop_last, collate_fn=list))

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        batches = self.index_batches()
        order = [i for b in batches for i in b]
        chunks = [order[k:k + self.chunk] for k in range(0, len(order), self.chunk)]
        ds = self.dataset
        done = []                    # per-sample tuples, in sample order
        done_act = []                # their raw pushes [T-1, 4]: attached to the collated batch
        bi = 0
        with ThreadPoolExecutor(max_workers=self.threads) as pool:
            pending = [pool.submit(ds.load, i) for i in chunks[0]] if chunks else []
            for k in range(len(chunks)):
                samples = [f.result() for f in pending]
                pending = [pool.submit(ds.load, i) for i in chunks[k + 1]] if k + 1 < len(chunks) else []
                draws = [ds.draw(s) for s in samples]
                done.extend(ds.tuples(samples, draws))
                done_act.extend(s['actions'] for s in samples)
                while bi < len(batches) and len(done) >= len(batches[bi]):
                    nb = len(batches[bi])
                    yield ds.collate(done[:nb], done_act[:nb])
                    done, done_act = done[nb:], done_act[nb:]
                    bi += 1

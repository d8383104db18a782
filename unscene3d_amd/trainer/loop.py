"""The self-training loop as a product: what `bench.py` assembles by hand around `InstanceSegmentation.training_step`
(reference: PyTorch-Lightning's fit loop around trainer/trainer.py:99-163, resumed from `last-epoch.ckpt`,
main_instance_segmentation.py:46-49, with `ModelCheckpoint(monitor="val_mean_ap_50", mode="max")`).

`TrainLoop` owns, in the order the benchmark does them: the flat gradient buffer and `FlatAdamW` over the parameters
that receive gradients, `OneCycleLR` stepped per batch, the captured decoder passes, the device collate, the gradient
reducer (world > 1, or `force_dist` over a one-rank group), the optimizer inside the backward pass, the
`ScenePrefetcher` with two batches in flight, the interpreter-lock switch interval, `StepsInFlight(2)`, and
`prepare_steady_state` after the first steps.  On top of that: a skipped batch costs nothing, the weighted losses reach
the host through a pinned ring without a wait, the whole training state can be saved and resumed to the bit, and a
validation pass runs every `check_val_every_n_epoch` epochs.

One program for every world size: under a reducer the optimizer is triggered by the reduced buckets
(`FlatAdamW.enable_early_reduced`, `usc_adamw_step_scaled` on the sum), without one by the step program's reports
(`FlatAdamW.enable_early`)."""
from __future__ import annotations

import collections
import os
import sys

import numpy as np
import torch

from .trainer import InstanceSegmentation, StepsInFlight, prepare_steady_state

LOSS_RING_SLOTS = 8           # > steps in flight + the entries a reader may still be looking at
MONITOR = "val_mean_ap_50"    # the reference's ModelCheckpoint monitor (mode "max")


def pin_to_device_numa(device):
    """Bind every thread of this process to the CPUs of the NUMA node the device hangs off (what a launcher does for a
    rank on a two-socket box; `bench.py` does the same for its own process).  USC3D_NUMA_PIN=0 leaves the affinity alone.
    -> the CPU list it bound to, or None."""
    if os.environ.get("USC3D_NUMA_PIN", "1") != "1" or not hasattr(os, "sched_setaffinity"):
        return None
    try:
        p = torch.cuda.get_device_properties(device)
        bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        with open(f"/sys/bus/pci/devices/{bdf}/local_cpulist") as f:
            text = f.read().strip()
        cpus = set()
        for part in text.split(","):
            if part:
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
        before = os.sched_getaffinity(0)
        cpus &= before
        if len(cpus) >= 8 and cpus != before:
            for tid in os.listdir("/proc/self/task"):
                try:
                    os.sched_setaffinity(int(tid), cpus)
                except OSError:
                    pass
            return text
    except (OSError, ValueError, AttributeError):
        pass
    return None


def _rng_snapshot(device):
    return {"torch": torch.get_rng_state(), "device": torch.cuda.get_rng_state(device), "numpy": np.random.get_state()}


def _rng_restore(snap, device):
    torch.set_rng_state(snap["torch"])
    torch.cuda.set_rng_state(snap["device"], device)
    np.random.set_state(snap["numpy"])


class TrainLoop:
    """loop = TrainLoop(module, cfg, scenes, device=dev);  loop.step() per batch, or loop.run(epochs=…).

    module: `InstanceSegmentation` on `device`, in train().  scenes: a sequence of raw scene tuples as
    `SyntheticFreeMaskDataset` / `FreeMaskDataset` yield them (indexed when a batch is issued, so a dataset that
    augments in `__getitem__` draws in batch order).  Order per epoch: `BucketedDistributedSampler` when world > 1
    (`sizes`: one number per scene, default the point counts), a seeded permutation otherwise (`shuffle=False`: index
    order).  world > 1 and `force_dist` need an initialised process group.

    total_steps / epochs: the length of the OneCycleLR schedule (total_steps wins; epochs defaults to
    cfg.trainer.max_epochs).  early_optimizer=False: one AdamW launch at the end of the step (under a reducer: the
    reducer averages, as before).  resident=True keeps the raw scene arrays in device memory (the collate reads them
    from there).  val_scenes + val_gt_ids ({scene name: ids}) switch the validation pass on; out_dir receives
    `last-epoch.ckpt` / `best.ckpt`.  collate: the train-mode collate function (default `FreeMaskVoxelizeCollate`;
    `datasets.utils.VoxelizeCollate(mode="train", …)` for scenes with ground-truth label tables)."""

    def __init__(self, module, cfg, scenes, *, device, world=1, rank=0, force_dist=False, early_optimizer=True,
                 overlap_allreduce=True, write_back_grad=False, batch_size=1, seed=0, shuffle=True, sizes=None,
                 bucket_window=8, total_steps=None, epochs=None, steady_after=2, steps_in_flight=None, prefetch_depth=2,
                 prefetch_thread=True, decoder_graphs=True, resident=False, spatial_sort=0, val_scenes=None,
                 val_gt_ids=None, out_dir=None, collate=None):
        from .. import ops
        from ..datasets.prefetch import ScenePrefetcher
        from ..datasets.utils import FreeMaskVoxelizeCollate
        from ..models import mask3d as _m3d

        if not isinstance(module, InstanceSegmentation):
            raise TypeError("TrainLoop: module must be a trainer.InstanceSegmentation")
        if len(scenes) == 0:
            raise ValueError("TrainLoop: no scenes")
        self.module, self.cfg, self.scenes = module, cfg, scenes
        self.device = dev = torch.device(device)
        self.world, self.rank, self.batch_size = int(world), int(rank), max(1, int(batch_size))
        self.dist = self.world > 1 or bool(force_dist)
        if self.dist:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError("TrainLoop: world > 1 / force_dist need an initialised process group")
            if dist.get_world_size() != self.world:
                raise RuntimeError(f"TrainLoop: world={self.world} but the process group has {dist.get_world_size()} ranks")
        self.seed, self.shuffle = int(seed), bool(shuffle)
        self.steady_after, self.steady = int(steady_after), None
        self.out_dir = out_dir
        self.val_scenes, self.val_gt_ids = val_scenes, val_gt_ids
        self._closed = False

        # ---- order of an epoch
        self.sampler = None
        if self.world > 1:
            from ..datasets.sampler import BucketedDistributedSampler
            if sizes is None:
                sizes = [len(self._peek_points(i)) for i in range(len(scenes))]
            self.sampler = BucketedDistributedSampler(sizes, self.world, self.rank, batch_size=self.batch_size,
                                                      window=max(1, int(bucket_window)), shuffle=self.shuffle, seed=self.seed)
            self.steps_per_epoch = len(self.sampler)
        else:
            self.steps_per_epoch = -(-len(scenes) // self.batch_size)

        # ---- optimizer + schedule over the parameters that receive gradients
        if total_steps is None:
            total_steps = self.steps_per_epoch * int(epochs or cfg.trainer.max_epochs)
        self.optimizer, self.scheduler, self.flat_grad = module.configure_optimizers(
            self.steps_per_epoch, epochs, flat=True, total_steps=int(total_steps))
        self.params = self.optimizer._params
        self._resident = {} if resident else None
        if decoder_graphs:
            module.model.enable_decoder_graphs(batch_size=self.batch_size, device=dev)
        self.collate = collate if collate is not None else FreeMaskVoxelizeCollate(
            ignore_label=255, voxel_size=cfg.data.voxel_size, mode="train", device=str(dev), spatial_sort=spatial_sort)

        # ---- gradient exchange, optimizer in the backward pass
        self.reducer = None
        reduced = self.dist and early_optimizer and overlap_allreduce
        if self.dist and overlap_allreduce:
            from ..ddp import BucketedGradReducer
            self.reducer = BucketedGradReducer(self.params, self.flat_grad, self.world, average=not reduced).install()
        self.early = None
        if reduced:
            self.optimizer.enable_early_reduced(self.reducer, write_back_grad=write_back_grad)
            self.early = "reduced"
        elif not self.dist and early_optimizer and getattr(_m3d, "_KV_SIDE_STREAM", False):
            self.optimizer.enable_early(module.model._side_stream(dev))
            self.early = "final"

        # ---- state of the run
        self.global_step = self.skipped = self.batches = 0
        self.epoch = self.pos = 0                 # the next batch to TAKE is number `pos` of epoch `epoch`
        self.best = None
        self.last_loss = self.last_losses = None  # device tensors of the last step (no read-back): total, weighted vector
        self._loss_keys = None
        self._ring = torch.zeros(LOSS_RING_SLOTS, 64, dtype=torch.float32).pin_memory()     # ONE pinned allocation
        self._ring_entries = collections.deque(maxlen=LOSS_RING_SLOTS - 2)    # (event, slot, step, n) newest last
        self._ring_next = 0

        # ---- batches ahead of the step
        self._depth = max(0, int(prefetch_depth))
        if steps_in_flight is None:
            steps_in_flight = int(os.environ.get("USC3D_STEPS_IN_FLIGHT", "2"))
        self.prefetch = None
        self._snaps = collections.deque()         # generator states in front of every batch issued and not yet taken
        if self._depth > 0:
            self.prefetch = ScenePrefetcher(self._issue_collate, add_raw_coordinates=cfg.data.add_raw_coordinates,
                                            device=dev, precompute=module.model.precompute_geometry,
                                            threaded=bool(prefetch_thread), bounded_lifetime=steps_in_flight > 0)
        self._ahead = (self.epoch, self.pos)      # the next batch to SUBMIT
        self._orders = {}
        self._start_prefetch()
        self._switch_interval = sys.getswitchinterval()
        ms = float(os.environ.get("USC3D_GIL_SWITCH_MS", "0.5"))
        if ms > 0:                                # two threads issue device work: the step and the next batches
            sys.setswitchinterval(ms / 1e3)
        self.in_flight = StepsInFlight(steps_in_flight)
        self._ops = ops

    # ------------------------------------------------------------------ scenes
    def _peek_points(self, i):
        return self.scenes[i][0]

    def _order(self, epoch):
        """Scene indices of this rank, [steps_per_epoch][batch_size], for one epoch."""
        got = self._orders.get(epoch)
        if got is None:
            if self.sampler is not None:
                got = self.sampler.plan(epoch)[:, self.rank, :].tolist()
            else:
                n = len(self.scenes)
                idx = (np.random.default_rng([self.seed, epoch]).permutation(n) if self.shuffle else np.arange(n)).tolist()
                total = self.steps_per_epoch * self.batch_size
                idx = (idx * (-(-total // n)))[:total]          # wrap-around padding, DistributedSampler's rule
                got = [idx[j:j + self.batch_size] for j in range(0, total, self.batch_size)]
            self._orders = {epoch: got}
        return got

    def _fetch(self, i):
        if self._resident is None:
            return self.scenes[i]
        got = self._resident.get(i)
        if got is None:
            got = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
                        if isinstance(x, np.ndarray) and j in (0, 1, 2) else x for j, x in enumerate(self.scenes[i]))
            self._resident[i] = got
        return got

    def _issue_collate(self, indices):
        """The prefetcher's collate: everything random about a batch (a dataset's augmentation, the collate's, the
        decoder's key samples drawn by precompute_geometry) is drawn behind this point, on the issuing thread, one batch
        at a time — the generator states in front of it are what a checkpoint needs to re-issue the batch."""
        self._snaps.append(_rng_snapshot(self.device))
        return self.collate([self._fetch(int(i)) for i in indices])

    def _advance(self, epoch, pos):
        pos += 1
        return (epoch + 1, 0) if pos >= self.steps_per_epoch else (epoch, pos)

    def _submit_next(self):
        e, p = self._ahead
        self.prefetch.submit(self._order(e)[p])
        self._ahead = self._advance(e, p)

    def _start_prefetch(self):
        self._ahead = (self.epoch, self.pos)
        if self.prefetch is not None:
            for _ in range(self._depth):
                self._submit_next()

    def _take(self):
        if self.prefetch is not None:
            batch = self.prefetch.take()
            self._snaps.popleft()
            return batch
        return self.collate([self._fetch(int(i)) for i in self._order(self.epoch)[self.pos]])

    def _quiesce_prefetch(self):
        """Wait until every submitted batch has been issued (their generator snapshots exist)."""
        if self.prefetch is not None:
            for box in self.prefetch._pending:
                if isinstance(box, dict):
                    box["done"].wait()

    # ------------------------------------------------------------------ one batch
    def step(self):
        """One batch: -> the total weighted loss (a device tensor, not read back), or None when the batch was skipped
        (no targets / a single-point level: no backward, no optimizer step, no scheduler step; `skipped` counts it).
        Between ranks a skip is this rank's alone, as in the reference: the scenes of a multi-rank run must have targets."""
        if self._closed:
            raise RuntimeError("TrainLoop.step() after close()")
        self.in_flight.begin()                    # at most two steps queued on the device
        batch = self._take()
        self.batches += 1
        self.epoch, self.pos = self._advance(self.epoch, self.pos)
        out = self.module.training_step(batch)
        if out is None:
            self.skipped += 1
        else:
            total, losses = out
            self.optimizer.zero_grad(set_to_none=False)
            if self.reducer is not None:
                self.reducer.begin_step()
            total.backward()
            if self.reducer is not None:
                self.reducer.finish()             # what backward has not already started; waits, averages unless reduced
            elif self.dist:
                import torch.distributed as dist
                dist.all_reduce(self.flat_grad)
                self.flat_grad.div_(self.world)
            self.optimizer.step()
            self.scheduler.step()
            self.global_step += 1
            self._report(total, losses)
        step_done = self.in_flight.end()
        if self.prefetch is not None:
            if self.prefetch.bounded:
                if step_done is None:
                    step_done = torch.cuda.Event()
                    step_done.record()
                self.prefetch.retire(step_done)   # this step's batch may go once the device is past this point
            self._submit_next()
        if self.steady is None and self.steady_after > 0 and self.global_step >= self.steady_after:
            self.steady = prepare_steady_state(self.device)
        return None if out is None else self.last_loss

    def _report(self, total, losses):
        """The weighted loss vector -> a slot of the pinned ring: one asynchronous copy and one event, no wait."""
        vals = list(losses.values())
        base = vals[0]._base if vals else None
        if base is None or base.dim() != 1 or base.numel() != len(vals):
            base = torch.stack(vals)
        vec = base.detach()
        self.last_loss, self.last_losses, self._loss_keys = total.detach(), vec, list(losses)
        n = vec.numel()
        if n > self._ring.shape[1]:
            raise RuntimeError(f"TrainLoop: {n} losses, the ring holds {self._ring.shape[1]} per step")
        slot = self._ring_next
        self._ring_next = (slot + 1) % LOSS_RING_SLOTS
        self._ring[slot, :n].copy_(vec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring_entries.append((ev, slot, self.global_step, n))

    def losses(self):
        """The newest reported step whose copy has completed: {"step": k, "losses": {name: float}}, or None when none
        has yet.  Never waits and queues nothing."""
        for ev, slot, step, n in reversed(self._ring_entries):
            if ev.query():
                row = self._ring[slot, :n].tolist()
                return {"step": step, "losses": dict(zip(self._loss_keys, row))}
        return None

    # ------------------------------------------------------------------ epochs, validation
    def run(self, epochs=None, max_steps=None):
        """Train `epochs` more epochs (or until `max_steps` batches were taken in this call), validating every
        cfg.trainer.check_val_every_n_epoch epochs when validation scenes were given.  -> a summary dict."""
        if epochs is None and max_steps is None:
            raise ValueError("TrainLoop.run: give epochs or max_steps")
        taken, metrics = 0, {}
        end_epoch = None if epochs is None else self.epoch + int(epochs)
        while (end_epoch is None or self.epoch < end_epoch) and (max_steps is None or taken < max_steps):
            before = self.epoch
            self.step()
            taken += 1
            if self.epoch != before:
                metrics = self.end_epoch() or metrics
        return {"steps": self.global_step, "skipped": self.skipped, "epoch": self.epoch, "metrics": metrics,
                "best": self.best}

    def end_epoch(self):
        """Called when the last batch of an epoch has been taken: the validation pass when it is due, `best.ckpt` when
        val_mean_ap_50 improved, `last-epoch.ckpt` always (out_dir).  -> the validation metrics ({} when none ran)."""
        done = self.epoch                          # epochs finished so far
        metrics = {}
        every = int(getattr(self.cfg.trainer, "check_val_every_n_epoch", 1) or 1)
        if self.val_scenes is not None and self.val_gt_ids is not None and done % every == 0:
            metrics = self.validate()
            score = metrics.get(MONITOR)
            if score is not None and (self.best is None or score > self.best):
                self.best = float(score)
                if self.out_dir is not None and self.rank == 0:
                    self.save_checkpoint(os.path.join(self.out_dir, "best.ckpt"))
        if self.out_dir is not None and self.rank == 0:
            self.save_checkpoint(os.path.join(self.out_dir, "last-epoch.ckpt"))
        return metrics

    def validate(self):
        """One pass over the validation scenes (begin_validation / validation_step / validation_epoch_end); the module
        is back in train() afterwards and the captured decoder passes are untouched (evaluation never replays them:
        its key sets are not sub-sampled, so the shape check sends every pass down the eager path)."""
        from ..datasets.utils import FreeMaskVoxelizeCollate
        collate = FreeMaskVoxelizeCollate(ignore_label=255, voxel_size=self.cfg.data.voxel_size, mode="validation",
                                          device=str(self.device))
        was_training = self.module.training
        self.module.eval()
        try:
            self.module.begin_validation(gt_ids=self.val_gt_ids)
            for i in range(len(self.val_scenes)):
                self.module.validation_step(collate([self.val_scenes[i]]), i)
            return self.module.validation_epoch_end()
        finally:
            self.module.train(was_training)

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """Everything the next batch depends on.  The generator states are those in front of the oldest batch that was
        issued ahead and not yet consumed: a resumed loop re-issues from there and draws what this one drew."""
        if self.reducer is not None:
            self.reducer.flush()                   # late-write flags of the last steps, before anything is written
        self._quiesce_prefetch()
        snap = self._snaps[0] if self._snaps else _rng_snapshot(self.device)
        return {"state_dict": self.module.state_dict(), "optimizer": self.optimizer.state_dict(),
                "lr_scheduler": self.scheduler.state_dict(), "global_step": self.global_step, "epoch": self.epoch,
                "position": self.pos, "batches": self.batches, "skipped": self.skipped, "best": self.best,
                "rng": snap, "loop": {"seed": self.seed, "shuffle": self.shuffle, "world": self.world,
                                      "batch_size": self.batch_size, "scenes": len(self.scenes)}}

    def load_state_dict(self, state, weights_only=None):
        """A checkpoint of this loop, or — weights only — a reference-format dict {"state_dict": {"model.…": …}} (the
        key contract of tests/golden/state_dict_keys.json).  weights_only=None: decided by what the dict holds."""
        sd = state["state_dict"]
        res = self.module.load_state_dict(sd, strict=False)        # in place: the flat parameter views stay
        bad = [k for k in list(res.missing_keys) + list(res.unexpected_keys) if k.startswith("model.")]
        if bad:
            raise RuntimeError(f"TrainLoop.load_state_dict: model keys do not match the checkpoint: {bad[:6]}")
        if weights_only is None:
            weights_only = "optimizer" not in state
        if weights_only:
            return
        meta = state.get("loop", {})
        mine = {"seed": self.seed, "shuffle": self.shuffle, "world": self.world, "batch_size": self.batch_size,
                "scenes": len(self.scenes)}
        if meta and meta != mine:
            raise RuntimeError(f"TrainLoop.load_state_dict: the checkpoint was written by a loop with {meta}, this one "
                               f"has {mine}: the position in the epoch would name other scenes")
        self.optimizer.load_state_dict(state["optimizer"])
        self.scheduler.load_state_dict(state["lr_scheduler"])
        self.global_step, self.epoch, self.pos = int(state["global_step"]), int(state["epoch"]), int(state["position"])
        self.batches, self.skipped, self.best = int(state["batches"]), int(state["skipped"]), state["best"]
        if self.steady_after > 0 and self.global_step >= self.steady_after:
            self.steady_after = self.global_step + 1          # the pools of THIS process are sized after its own first step
        # drop what was issued ahead for the old position, rewind the generators, issue again from the new one
        if self.prefetch is not None:
            self._quiesce_prefetch()
            self.prefetch.drain()
            self._snaps.clear()
        _rng_restore(state["rng"], self.device)
        self._start_prefetch()

    def save_checkpoint(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = f"{path}.tmp"
        torch.save(self.state_dict(), tmp)
        os.replace(tmp, path)                      # never a half-written last-epoch.ckpt

    @classmethod
    def resume(cls, path, module, cfg, scenes, **kw):
        """A loop built like the one that wrote `path`, continued from there."""
        loop = cls(module, cfg, scenes, **kw)
        try:
            loop.load_state_dict(torch.load(path, map_location="cpu", weights_only=False))
        except BaseException:
            loop.close()
            raise
        return loop

    # ------------------------------------------------------------------ end
    def close(self):
        """Stop the prefetch worker, take the optimizer out of the backward pass and remove the hooks this loop set in
        `ops`: a second loop — or a test — after it starts clean."""
        if self._closed:
            return
        self._closed = True
        ops = self._ops
        if self.prefetch is not None:
            self.prefetch.close()
        torch.cuda.synchronize(self.device)       # nothing of a running step is cut off below
        self.optimizer._early_done, self.optimizer._joins = [], []
        self.optimizer.disable_early()
        if ops.PARAMS_FINAL_HOOK is not None and getattr(ops.PARAMS_FINAL_HOOK, "__self__", None) is self.optimizer:
            ops.PARAMS_FINAL_HOOK = None
        if self.reducer is not None:
            if getattr(ops.GRAD_WRITTEN_HOOK, "__self__", None) is self.reducer:
                ops.GRAD_WRITTEN_HOOK = None
            for h in self.reducer._hooks:
                h.remove()
        sys.setswitchinterval(self._switch_interval)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def fit(cfg, scenes, *, device="cuda", module=None, seed=1234, epochs=None, max_steps=None, resume=None, **kw):
    """Build the module (unless given), run the loop, close it.  epochs: how many to train in this call (default: up to
    cfg.trainer.max_epochs); resume: a checkpoint written by `TrainLoop.save_checkpoint`.
    -> (module, summary dict of TrainLoop.run)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if module is None:
        torch.manual_seed(seed)
        module = InstanceSegmentation(cfg).to(dev).train()
    make = (lambda: TrainLoop.resume(resume, module, cfg, scenes, device=dev, **kw)) if resume else \
        (lambda: TrainLoop(module, cfg, scenes, device=dev, **kw))
    with make() as loop:
        if epochs is None and max_steps is None:
            epochs = max(0, int(cfg.trainer.max_epochs) - loop.epoch)
        out = loop.run(epochs=epochs, max_steps=max_steps)
        torch.cuda.synchronize(dev)
        out["losses"] = loop.losses()
    return module, out

"""MF trainer with the entry points of the reference's ``src/matrix_factorization/torch_trainer.py``:

    python torch_trainer.py <config_path relative to settings.MODELS>          (``:166-170``)

``train()`` (``:24-84``) and ``validate()`` (``:87-161``) keep their signatures and return values;
the per-batch body runs in fused HIP kernels (``otto_mf_step_sparse_adam`` / ``otto_mf_eval``) and the
per-batch ``loss.item()`` host sync (``:78``, ``:137``) is replaced by ONE read at the end of the epoch.
YAML schema: ``models/matrix_factorization/config.yaml``, ``models/aid_collaborative_filtering/config.yaml``.
Reference defects of SURVEY.md App. E (NameError on ``df_session_aids``, KeyError on
``mean_absolute_error``, off-by-one ``best_epoch``) are not reproduced.
"""
import argparse
import logging
import pathlib
import sys

import numpy as np
import torch
import torch.nn
import torch.optim as optim
import yaml

if __package__ in (None, ''):   # run as a script from its own directory, like the reference
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import otto_amd.matrix_factorization  # noqa: F401
    __package__ = 'otto_amd.matrix_factorization'

from .. import settings
from . import torch_modules, torch_utils, torch_optim, metrics, visualization
from .data import DeviceBatchLoader, build_aid_pairs_device, build_sessions_aids  # noqa: F401
from . import distributed as dd
from .distributed import DataParallelSparseAdam, ShardedBatchLoader, full_state_dict
from .torch_optim import loss_kind


def _unpack(model, inputs, device):
    if isinstance(model, torch_modules.CollaborativeFiltering):
        keys = ('x1', 'x2')
    elif isinstance(model, torch_modules.MatrixFactorization):
        keys = ('session', 'aid')
    else:
        raise ValueError('Invalid model')
    cvt = lambda t: t.to(device=device, dtype=torch.int64).contiguous()
    return cvt(inputs[keys[0]]), cvt(inputs[keys[1]]), cvt(inputs['target'])


class _LossLog:
    """Per-batch losses stay on the device; read once per epoch."""

    def __init__(self, device):
        self.buf = torch.empty(4096, dtype=torch.float32, device=device)
        self.n = 0

    def slot(self):
        if self.n == self.buf.numel():
            self.buf = torch.cat((self.buf, torch.empty_like(self.buf)))
        self.n += 1
        return self.buf[self.n - 1:self.n]

    def values(self):
        return self.buf[:self.n].cpu().numpy().astype(np.float64)


def train(train_loader, model, criterion, optimizer, device, scheduler=None):
    """Train ``model`` for one pass over ``train_loader``; returns the mean of the batch losses
    (reference ``train()``, ``torch_trainer.py:24-84``).  ``optimizer`` must be
    ``torch_optim.SparseAdam`` (what the reference's configs name).

    Data parallel: a :class:`~.distributed.DataParallelSparseAdam` with a :class:`~.distributed.ShardedBatchLoader`;
    every step is the global batch's step, and the epoch's loss is combined with one all-reduce, so every rank returns
    the same number."""
    if not isinstance(optimizer, torch_optim.SparseAdam):
        raise ValueError('the fused trainer supports optimizer: SparseAdam (models/*/config.yaml)')
    dp = isinstance(optimizer, DataParallelSparseAdam)
    if dp != isinstance(train_loader, ShardedBatchLoader):
        raise ValueError('data-parallel training needs both DataParallelSparseAdam and ShardedBatchLoader')
    model.train()
    log = _LossLog(torch.device(device))
    for k, (inputs, _) in enumerate(train_loader):
        i1, i2, targets = _unpack(model, inputs, device)
        step = dict(batch_global=train_loader.batch_global(k), private_rows=train_loader.private_rows,
                    max_local_batch=train_loader.max_local_batch) if dp else {}
        optimizer.fused_step(model, i1, i2, targets, criterion, log.slot(), **step)
        if scheduler is not None:
            scheduler.step()
    if log.n:
        model.engine(1).check()          # out-of-range row ids were skipped in the kernels: raise here, once per epoch
    # data parallel: each step's value is this rank's loss sum / B_global, so the ranks' sums add up to the step's mean loss
    total = log.values().sum()
    if dp and log.n:
        total = optimizer.all_reduce_sum([total])[0]
    return float(total / log.n) if log.n else float('nan')


def validate(val_loader, model, criterion, device, scores=False):
    """Validation loss (mean of batch means) and, with ``scores``, the score dict of
    ``metrics.regression_scores`` / ``classification_scores`` (reference ``validate()``, ``:87-161``).

    The reference moves every batch's predictions to the host and scores them with scikit-learn (``:144-158``); here the
    eval kernel keeps running sums (MAE, MSE, accuracy) and only the classification model's ROC-AUC needs the predictions,
    which stay on the device for one sort.

    With a :class:`~.distributed.ShardedBatchLoader` each rank evaluates its shard: batch losses are weighted by
    ``B_local / B_global`` and summed over ranks, the running sums are all-reduced, and ROC-AUC is computed from the
    all-gathered predictions; every rank returns the same values."""
    sharded = isinstance(val_loader, ShardedBatchLoader)
    model.eval()
    dev = torch.device(device)
    log = _LossLog(dev)
    kind = loss_kind(criterion)
    E1, E2, _ = model._tables()
    classification = isinstance(model, torch_modules.CollaborativeFiltering)
    truth, predictions, eng = [], [], None
    if sharded:         # every rank takes part in the collectives below, with or without rows of its own
        eng = model.engine(max(val_loader.max_local_batch, 1))
        if scores:
            eng.read_sums(reset=True)
    with torch.no_grad():
        for k, (inputs, _) in enumerate(val_loader):
            i1, i2, targets = _unpack(model, inputs, device)
            slot, B = log.slot(), i1.numel()
            if B == 0:      # a rank's share of a step may be empty
                slot.zero_()
                continue
            if eng is None and scores:
                model.engine(B).read_sums(reset=True)       # start the epoch's running sums from zero
            eng = model.engine(B)
            pred = torch.empty(B, dtype=torch.float32, device=dev) if scores and classification else None
            (eng.eval_sums if scores else eng.eval)(E1.data, E2.data, i1, i2, targets, kind, slot, pred)
            if sharded:
                slot.mul_(B / val_loader.batch_global(k))
            if pred is not None:
                truth.append(targets)
                predictions.append(pred)
    if eng is not None:
        eng.check()
    red = [log.values().sum()] + (list(eng.read_sums(reset=True)) if scores and eng is not None else [])
    if sharded and val_loader.world > 1:
        red = dd._all_reduce(torch.tensor(red, dtype=torch.float64), dd.dist.ReduceOp.SUM, val_loader.group,
                             val_loader.stage).tolist()
    val_loss = float(red[0] / log.n) if log.n else float('nan')
    val_scores = None
    if scores and eng is not None:
        auc = None
        if classification:
            t_all, p_all = _gather_sharded(val_loader, truth, predictions, dev) if sharded else \
                (torch.cat(truth), torch.cat(predictions))
            auc = metrics.roc_auc(t_all, torch.sigmoid(p_all))
        val_scores = metrics.scores_from_sums(tuple(red[1:5]), classification, auc)
    return val_loss, val_scores


def _gather_sharded(loader, truth, predictions, dev):
    """Every rank's targets (as float32) and predictions, in rank order."""
    world, n_max = loader.world, max(loader.sizes)
    t_loc = torch.zeros(n_max, dtype=torch.float32, device=dev)
    p_loc = torch.zeros(n_max, dtype=torch.float32, device=dev)
    if truth:
        t_cat, p_cat = torch.cat(truth), torch.cat(predictions)
        t_loc[:t_cat.numel()] = t_cat.to(torch.float32)
        p_loc[:p_cat.numel()] = p_cat
    t_all = torch.empty((world, n_max), dtype=torch.float32, device=dev)
    p_all = torch.empty((world, n_max), dtype=torch.float32, device=dev)
    if world > 1:
        dd._all_gather(t_all, t_loc, loader.group, loader.stage)
        dd._all_gather(p_all, p_loc, loader.group, loader.stage)
    else:
        t_all[0], p_all[0] = t_loc, p_loc
    return (torch.cat([t_all[r, :n] for r, n in enumerate(loader.sizes)]),
            torch.cat([p_all[r, :n] for r, n in enumerate(loader.sizes)]))


def build_optimizer(name, params, args):
    """``getattr(optim, name)`` of the reference (``:352``) with SparseAdam mapped to the fused one."""
    if name == 'SparseAdam':
        return torch_optim.SparseAdam(params, **args)
    raise ValueError(f'optimizer {name} is not supported by the fused trainer (SparseAdam only)')


DISTRIBUTED_KEYS = {'backend', 'device'}


def _distributed_setup(config):
    """The optional ``training.distributed`` section: ``{backend: nccl | gloo, device: local_rank | configured}``. The
    process group comes from the ``RANK`` / ``WORLD_SIZE`` / ``MASTER_ADDR`` / ``MASTER_PORT`` environment a
    ``torchrun``-style launcher (``python -m torch.distributed.run``) sets. Returns None when the section is absent."""
    sec = config['training'].get('distributed')
    if sec is None:
        return None
    if not isinstance(sec, dict):
        raise ValueError('training.distributed must be a mapping such as {backend: nccl}')
    unknown = set(sec) - DISTRIBUTED_KEYS
    if unknown:
        raise ValueError(f'training.distributed: unsupported key(s) {sorted(unknown)} (supported: {sorted(DISTRIBUTED_KEYS)})')
    backend = sec.get('backend', 'nccl')
    if backend not in ('nccl', 'gloo'):
        raise ValueError(f"training.distributed.backend must be 'nccl' or 'gloo' (got {backend!r})")
    placement = sec.get('device', 'local_rank')
    if placement not in ('local_rank', 'configured'):
        raise ValueError(f"training.distributed.device must be 'local_rank' or 'configured' (got {placement!r})")
    if config['training']['optimizer'] != 'SparseAdam':
        raise ValueError('data-parallel training supports optimizer: SparseAdam only')
    import os
    missing = [k for k in ('RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT') if k not in os.environ]
    if missing:
        raise ValueError(f'training.distributed needs a torchrun-style launcher: {", ".join(missing)} not set '
                         '(python -m torch.distributed.run --nproc_per_node=N torch_trainer.py <config>)')
    import torch.distributed as dist
    device = torch.device(f'cuda:{int(os.environ.get("LOCAL_RANK", 0))}') if placement == 'local_rank' \
        else torch.device(config['training']['device'])
    torch.cuda.set_device(device)
    owned = not dist.is_initialized()
    if owned:
        dist.init_process_group(backend)
    return dict(backend=backend, device=device, rank=dist.get_rank(), world=dist.get_world_size(), owned=owned)


def run(config, df=None):
    """Everything below ``__main__`` in the reference (``torch_trainer.py:172-505``).

    With a ``training.distributed`` section (:func:`_distributed_setup`) every rank trains its shard with
    :class:`~.distributed.DataParallelSparseAdam`; rank 0 alone builds the dataset file, writes checkpoints (with every
    rank's session rows, :func:`~.distributed.full_state_dict`) and the learning curve. Without it nothing changes."""
    import pandas as pd
    dpc = _distributed_setup(config)
    try:
        return _run(config, df, pd, dpc)
    finally:
        if dpc is not None and dpc['owned']:
            import torch.distributed as dist
            dist.destroy_process_group()


def _run(config, df, pd, dpc):
    lead = dpc is None or dpc['rank'] == 0
    cls = config['model']['model_class']
    if cls == 'CollaborativeFiltering':
        root, fname, score_keys = pathlib.Path(settings.DATA / 'collaborative_filtering'), 'aid_pairs.parquet', ('accuracy', 'roc_auc')
    elif cls == 'MatrixFactorization':
        root, fname, score_keys = pathlib.Path(settings.DATA / 'matrix_factorization'), 'sessions_aids.parquet', \
            ('mean_absolute_error', 'mean_squared_error')
    else:
        raise ValueError('Invalid model')
    root.mkdir(parents=True, exist_ok=True)
    if not config['dataset']['load_dataset'] and lead:
        if df is None:
            df = pd.concat((pd.read_pickle(settings.DATA / 'train.pkl'), pd.read_pickle(settings.DATA / 'test.pkl')),
                           axis=0, ignore_index=True)
        if cls == 'CollaborativeFiltering':
            # sort, self-join / shift-shuffle, de-duplication and per-pair aggregation on the device (include/otto_events.h,
            # include/otto_pairs.h); only the finished (x1, x2, target) rows come back for the parquet file
            from ..events import frame_to_events_device
            dsc = config['dataset']
            ev = frame_to_events_device(df, device=config['training']['device'])
            x1, x2, tg = build_aid_pairs_device(ev, dsc['sampling_strategy'], dsc.get('hour_difference', 1),
                                                dsc.get('target_aggregation', 'mean'), seed=config['training']['random_state'])
            ds = pd.DataFrame({'x1': x1.cpu().numpy(), 'x2': x2.cpu().numpy(), 'target': tg.cpu().numpy()})
            del ev, x1, x2, tg
        else:
            ds = build_sessions_aids(df)
        ds.to_parquet(root / fname)
        logging.info(f'{fname} is saved to {root}')
    elif lead:
        logging.info(f'Using pre-computed dataset from {root / fname}')
    if dpc is not None:
        import torch.distributed as dist
        dist.barrier()            # rank 0 has written the dataset file

    tr = config['training']
    device = torch.device(tr['device']) if dpc is None else dpc['device']
    torch_utils.set_seed(tr['random_state'], deterministic_cudnn=tr['deterministic_cudnn'])
    if dpc is None:
        train_loader = DeviceBatchLoader.from_parquet(root / fname, tr['training_batch_size'], shuffle=True, device=device,
                                                      seed=tr['random_state'])
        val_loader = DeviceBatchLoader(train_loader.columns, tr['validation_batch_size'], shuffle=True, device=device,
                                       seed=tr['random_state'] + 1)       # validation file == training file (reference :307-311)
    else:
        import pyarrow.parquet as pq
        table = pq.read_table(str(root / fname))
        cols = {n: table.column(n).to_numpy() for n in table.column_names if not n.startswith('__')}
        shard = dict(shard_key=None) if cls == 'CollaborativeFiltering' else \
            dict(shard_key='session', n_keys=config['model']['n_sessions'])
        train_loader = ShardedBatchLoader(cols, tr['training_batch_size'], shuffle=True, device=device, seed=tr['random_state'],
                                          **shard)
        val_loader = ShardedBatchLoader(cols, tr['validation_batch_size'], shuffle=True, device=device,
                                        seed=tr['random_state'] + 1, **shard)
        del table, cols
    model_root = pathlib.Path(settings.MODELS / config['persistence']['model_directory'])
    model_root.mkdir(parents=True, exist_ok=True)
    criterion = getattr(torch.nn, tr['loss_function'])(**tr['loss_args'])
    m = config['model']
    if cls == 'CollaborativeFiltering':
        model = torch_modules.CollaborativeFiltering(n_embeddings=m['n_embeddings'], n_factors=m['n_factors'], sparse=m['sparse'],
                                                     dropout_probability=m['dropout_probability'])
    else:
        model = torch_modules.MatrixFactorization(n_sessions=m['n_sessions'], n_aids=m['n_aids'], n_factors=m['n_factors'],
                                                  sparse=m['sparse'], dropout_probability=m['dropout_probability'])
    train_loader.check_ranges({'x1': m['n_embeddings'], 'x2': m['n_embeddings']} if cls == 'CollaborativeFiltering'
                              else {'session': m['n_sessions'], 'aid': m['n_aids']})
    if m['model_checkpoint_path'] is not None:
        model.load_state_dict(torch.load(m['model_checkpoint_path'], weights_only=True))
    model.to(device)
    optimizer = build_optimizer(tr['optimizer'], model.parameters(), tr['optimizer_args']) if dpc is None else \
        DataParallelSparseAdam(model.parameters(), **tr['optimizer_args'])
    state = (lambda: model.state_dict()) if dpc is None else (lambda: full_state_dict(model, train_loader))
    plateau = tr['lr_scheduler'] == 'ReduceLROnPlateau'
    scheduler = getattr(optim.lr_scheduler, tr['lr_scheduler'])(optimizer, **tr['lr_scheduler_args'])

    summary = {'train_loss': [], 'val_loss': [], **{f'val_{k}': [] for k in score_keys}}
    for epoch in range(1, tr['epochs'] + 1):
        train_loss = train(train_loader, model, criterion, optimizer, device, scheduler=None if plateau else scheduler)
        val_loss, val_scores = validate(val_loader, model, criterion, device, scores=tr['scores'])
        if plateau:
            scheduler.step(val_loss)
        logging.info(f'Epoch {epoch} - Training Loss: {train_loss:.4f} - Validation Loss: {val_loss:.4f} - '
                     + ' '.join(f'{k}: {v:.4f}' for k, v in (val_scores or {}).items()))
        if epoch in config['persistence']['save_epoch_model']:
            sd = state()          # collective in data-parallel runs: every rank takes part, rank 0 writes
            if lead:
                torch.save(sd, model_root / f'model_epoch_{epoch}.pt')
                logging.info(f'Saved model_epoch_{epoch}.pt to {model_root}')
        best_val_loss = np.min(summary['val_loss']) if len(summary['val_loss']) > 0 else np.inf
        if val_loss < best_val_loss and config['persistence']['save_best_model']:
            sd = state()
            if lead:
                torch.save(sd, model_root / 'model_best.pt')
                logging.info(f'Saved model_best.pt (validation loss decreased from {best_val_loss:.6f} to {val_loss:.6f})')
        summary['train_loss'].append(train_loss)
        summary['val_loss'].append(val_loss)
        for k in score_keys:
            summary[f'val_{k}'].append(val_scores[k] if val_scores else np.nan)
        best_epoch = int(np.argmin(summary['val_loss']))      # 0-based
        if tr['early_stopping_patience'] > 0 and len(summary['val_loss']) - 1 - best_epoch >= tr['early_stopping_patience']:
            logging.info(f'Early Stopping (validation loss didn\'t improve for {tr["early_stopping_patience"]} epochs) '
                         f'Best Epoch ({best_epoch + 1}) Validation Loss: {summary["val_loss"][best_epoch]:.4f}')
            break
    best_epoch = int(np.argmin(summary['val_loss']))
    scores = {'val_loss': summary['val_loss'][best_epoch], **{f'val_{k}': summary[f'val_{k}'][best_epoch] for k in score_keys}}
    if config['persistence']['visualize_learning_curve'] and lead:
        visualization.visualize_learning_curve(training_losses=summary['train_loss'], validation_losses=summary['val_loss'],
                                               validation_scores={f'val_{k}': summary[f'val_{k}'] for k in score_keys},
                                               path=str(model_root / 'learning_curve.png'))
        logging.info(f'Saved learning_curve.png to {model_root}')
    return model, summary, scores


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('config_path', type=str)
    args = parser.parse_args()
    config = yaml.load(open(settings.MODELS / args.config_path, 'r'), Loader=yaml.FullLoader)
    run(config)

"""``DATA/splits/{train,val}.parquet`` -> ``DATA/parquet_files/train_truncated_parquet/train_truncated_<i>.parquet``: the
reference's ``src/utilities/split_dataset_writer_parquet.py`` with decode, sort and encode on the device. Same ``settings``
shim, same files::

    OTTO_ROOT=/path/to/project python -m otto_amd.utilities.split_dataset_writer_parquet [--encoding plain|delta] [--compression snappy]

The two split files are decoded by ``otto_amd.parquet`` (SPEC-PARQUET), their columns raw, with no unit change; the rows are
sorted by (session, ts), stable, with torch (plumbing); chunk i holds the sessions whose *value* lies in
``[i * 100_000, (i + 1) * 100_000)``, as the reference's ``>=`` / ``<`` masks cut them, and there are
``nunique // 100_000 + 1`` chunks -- the reference's count, so a final empty chunk is written where it writes one. The files
are encoded by ``otto_amd.parquet_write`` (SPEC-PQWRITE). The dtypes read back are those of ``DataFrame.to_parquet`` of
the same frame; the pandas index metadata is not written, so ``pd.read_parquet`` yields the ``RangeIndex`` that
``reset_index(drop=True)`` leaves in the reference.

``--encoding plain`` (the default) writes PLAIN pages, which this project's own device decoder reads
(``parquet.read_columns``, ``builder.py validation --device-parquet``); ``--encoding delta`` writes DELTA_BINARY_PACKED
pages for the four integer columns, for size: pyarrow and pandas read them, and so does the device decoder
(``events.parquet_to_events_device`` gives the same events from either encoding). The default stays PLAIN.

``--compression snappy`` compresses every page on the device after its value encoding (``otto_amd.snappy``, SPEC-SNAPPY):
the codec of the reference's own files, read by pyarrow, pandas and the device decoder. Without it the files are
uncompressed, as before.
"""
import argparse
import logging
import pathlib

from .. import parquet, parquet_write, settings

SESSION_CHUNK_SIZE = 100_000


def read_split_columns(paths, device='cuda:0'):
    """``{name: device tensor}`` of every column of the split files, in file order, with the dtype the file declares
    (an unsigned column of 16 bits or more comes back from the decoder as the signed type of its width and is viewed)."""
    import torch
    from .. import _lib
    paths = [str(p) for p in paths]
    leaves = parquet.read_metadata(paths[0]).leaves
    names = [l.name for l in leaves]
    cols = parquet.read_columns(paths, names, device)
    out = {}
    for leaf, t in zip(leaves, cols):
        lg = leaf.logical
        if lg is not None and lg[0] != 'INT':
            raise _lib.OttoError(f'{paths[0]}: column {leaf.name!r}: logical type {lg} cannot be written back (SPEC-PQWRITE)')
        if lg and not lg[2] and lg[1] > 8:
            t = t.view(getattr(torch, f'uint{lg[1]}'))
        out[leaf.name] = t
    return out


def sort_and_cut(columns, chunk=SESSION_CHUNK_SIZE):
    """The columns sorted by (session, ts), stable, and the row cut points of the chunks."""
    import torch
    session, ts = columns['session'].long(), columns['ts'].long()
    order = torch.argsort(ts, stable=True)
    order = order[torch.argsort(session[order], stable=True)]
    signed = {torch.uint16: torch.int16, torch.uint32: torch.int32, torch.uint64: torch.int64}      # torch gathers these as signed

    def take(v):
        return v.view(signed[v.dtype])[order].view(v.dtype) if v.dtype in signed else v[order]
    columns = {k: take(v).contiguous() for k, v in columns.items()}
    session = session[order]
    n_chunks = int(torch.unique(session).numel()) // chunk + 1
    bounds = torch.arange(0, n_chunks + 1, device=session.device, dtype=torch.int64) * chunk
    cuts = torch.searchsorted(session, bounds).cpu().tolist()
    return columns, cuts


def write_chunks(paths, directory, device='cuda:0', encoding='plain', chunk=SESSION_CHUNK_SIZE, **kw):
    """The chunk files of the split files ``paths`` into ``directory``; returns their paths. ``compression='snappy'`` and the
    other keywords of ``parquet_write.write_tables`` pass through."""
    directory = pathlib.Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    columns, cuts = sort_and_cut(read_split_columns(paths, device), chunk)
    out = [directory / f'train_truncated_{i}.parquet' for i in range(len(cuts) - 1)]
    parquet_write.write_tables(out, columns, cuts, {k: encoding for k in columns}, **kw)
    return out


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--encoding', choices=('plain', 'delta'), default='plain')
    parser.add_argument('--compression', choices=('snappy',), default=None)
    args = parser.parse_args(argv)
    directory = settings.DATA / 'parquet_files' / 'train_truncated_parquet'
    out = write_chunks([settings.DATA / 'splits' / f'{name}.parquet' for name in ('train', 'val')], directory, encoding=args.encoding,
                       compression=args.compression)
    logging.info(f'{len(out)} train_truncated_<chunk_idx>.parquet files are saved to {directory}')


if __name__ == '__main__':
    main()

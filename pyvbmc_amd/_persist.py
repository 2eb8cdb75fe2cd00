"""Writing an object to a file and reading it back: what ``VBMC.save`` / ``load`` and ``VariationalPosterior.save`` /
``load`` share.

The format is a plain ``pickle`` of the whole object in ONE dump, so that what is shared between its parts (one
transformer across driver, posterior and logger; ``optim_state["hyp_dict"]`` and ``hyp_dict``) is shared again after the
load.  Where plain ``pickle`` refuses the object -- a target written as a lambda or a closure -- the dump is ``dill``'s, if
``dill`` imports; nothing installs it.  The write is atomic: a temporary file in the target's directory, flushed, then
``os.replace``; a process that is killed during the write leaves the file that was there before.

Loading a pickle runs code: load only files you wrote yourself.
"""
import os
import pickle
import tempfile
from pathlib import Path


def _import_dill():
    try:
        import dill
    except ImportError:
        return None
    return dill


def file_path(file):
    """``file`` as a path, with ``.pkl`` appended to a name that has no suffix (the reference's rule)."""
    path = Path(file)
    return path.with_suffix(".pkl") if path.suffix == "" else path


def save(obj, file, overwrite=False):
    """Write ``obj`` to ``file`` (module text); ``FileExistsError`` for an existing file unless ``overwrite``.  Returns
    the path written."""
    path = file_path(file)
    if not overwrite and path.exists():
        raise FileExistsError(f"{path} exists; pass overwrite=True to replace it")
    fd, tmp = tempfile.mkstemp(prefix=path.name + ".", suffix=".tmp", dir=path.parent)
    try:
        with os.fdopen(fd, "wb") as f:
            try:
                pickle.dump(obj, f, protocol=pickle.HIGHEST_PROTOCOL)
            except (pickle.PicklingError, AttributeError) as exc:
                dill = _import_dill()
                if dill is None:
                    raise TypeError(f"{type(obj).__name__}.save: {exc}.  Plain pickle takes functions by their module-level "
                                    "name only: define the target (and the prior) at module level, or install dill") from exc
                f.seek(0)
                f.truncate()
                dill.dump(obj, f, recurse=True)
            f.flush()
            os.fsync(f.fileno())
        if not overwrite and path.exists():
            raise FileExistsError(f"{path} exists; pass overwrite=True to replace it")
        os.replace(tmp, path)
    except BaseException:
        _unlink_quietly(tmp)
        raise
    return path


def _unlink_quietly(tmp):
    try:
        os.unlink(tmp)
    except OSError:
        pass


def load(file):
    """The object ``save`` wrote (``dill``'s loader where ``dill`` imports: it reads both kinds of dump)."""
    dill = _import_dill()
    with open(file_path(file), "rb") as f:
        return (dill or pickle).load(f)

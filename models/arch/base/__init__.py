"""Building blocks of the architectures: linear_group (LinearGroup), norm (new_norm and the group norms), retention (MultiScaleRetention, RetNetRelPos),
mamba (Mamba: the selective state-space block in plain torch with mamba_ssm's interface and state_dict keys, a port from the published equations; it stands
in for mamba_ssm, parity not pinned) and native (the switches and warnings of the native paths)."""

"""Mirror of the reference's evaluation/ package: what is drawn from a model's outputs."""
